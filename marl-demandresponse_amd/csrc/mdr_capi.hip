// mdr_capi.hip — C-ABI host runtime: contexts, launches, graph cache, greedy scratch, RCCL.
//
// The C ABI (include/mdr.h) is what the Python layer (mdr_amd, via ctypes) and any other host
// binds.  It owns only small scratch; every launch goes to the caller's stream.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <rccl/rccl.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "mdr_actor.h"
#include "mdr_devbuf.h"
#include "mdr_interp.h"
#include "mdr_obs_dev.h"
#include "mdr_kernels.h"
#include "mdr_validity.h"

using namespace mdr;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (expr);                                                                \
    if (e_ != hipSuccess)                                                                  \
      return fail(MDR_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));            \
  } while (0)

#define RCCL_TRY(expr)                                                                     \
  do {                                                                                     \
    ncclResult_t r_ = (expr);                                                              \
    if (r_ != ncclSuccess) return fail(MDR_ERCCL, std::string(#expr) + ": " + ncclGetErrorString(r_)); \
  } while (0)

#define LAUNCH_CHECK(what)                                                                 \
  do {                                                                                     \
    hipError_t e_ = hipGetLastError();                                                     \
    if (e_ != hipSuccess) return fail(MDR_EHIP, std::string(what) + ": " + hipGetErrorString(e_)); \
  } while (0)

// Device memory has one owner type (mdr_devbuf.h) and this one allocator: every buffer of a context
// is a Dev<T> member and goes with the context's destructor.  A site that grows a
// buffer queued work may still use: synchronise, drop the cached graphs that hold its address, then
// reserve, which frees before it allocates and is empty in between.  What a captured launch sequence
// uses is reserved, and zero-filled by hipMemset (never a memset node: zero_slabs), before the capture.
struct HipAlloc {
  static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
};
template <class T>
using Dev = DevBuf<T, HipAlloc>;

// room for n elements, zero-filled if asked and newly allocated; a failure is MDR_EHIP with the buffer's
// name (mdr_create and mdr_interp_load report MDR_ENOMEM in words of their own: they call reserve)
template <class T>
int dev_reserve(Dev<T>& b, size_t n, const char* name, bool zero = false) {
  if (n <= b.capacity()) return MDR_OK;
  hipError_t e = (hipError_t)b.reserve(n);
  if (e == hipSuccess && zero && (e = hipMemset(b, 0, n * sizeof(T))) != hipSuccess) b.reset();
  return e == hipSuccess ? MDR_OK : fail(MDR_EHIP, std::string(name) + ": " + hipGetErrorString(e));
}
template <class T>
size_t dev_bytes(const Dev<T>& b) { return b.capacity() * sizeof(T); }

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline unsigned blocks(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

// the wave tiles (64 x kWinHpt houses) of a shard, and tiles rounded up to whole blocks of `waves`
// waves (a tile per wave): the window kernels' grids and every buffer sized by them
inline size_t win_tiles(int64_t n) { return ((size_t)n + 64 * kWinHpt - 1) / (64 * kWinHpt); }
inline size_t whole_blocks(size_t tiles, int waves) { return (tiles + waves - 1) / waves * waves; }

// n ticks as ceil(n / win) windows of near-equal size, the larger ones first
struct WinPlan {
  int nw, base, rem;
  WinPlan(int n, int win) : nw((n + win - 1) / win), base(n / nw), rem(n % nw) {}
  int count() const { return nw; }
  int size(int w) const { return base + (w < rem ? 1 : 0); }
  int start(int w) const { return w * base + (w < rem ? w : rem); }
};

// what every rollout entry point hands to its launch sequence
struct RolloutArgs {
  int n;
  const uint8_t* action;
  int64_t act_stride;
  int mode;
  double* reward;
  int64_t rew_stride;
  double* p_out;
  const uint8_t* act_row(int t) const { return action ? action + (int64_t)t * act_stride : nullptr; }
  double* rew_row(int t) const { return reward + (int64_t)t * rew_stride; }
};

struct GraphKey {
  RolloutArgs a;
  void* stats;  // mdr_rollout_stats: the rows' buffer and the first row (baked into the launches)
  int row0;
  auto fields() const {
    return std::tie(a.n, a.mode, a.action, a.act_stride, a.reward, a.rew_stride, a.p_out, stats, row0);
  }
  bool operator<(const GraphKey& o) const { return fields() < o.fields(); }
};

// what the six actor rollout entry points hand to the single-GPU or the sharded function
struct ActorRolloutArgs {
  int n; const mdr_tick* ticks;
  const mdr_obs_scalars* osc; const mdr_obs_spec* sp;
  uint8_t* action; int64_t act_stride;
  float* prob; int64_t prob_stride;
  double* reward; int64_t rew_stride; double* p_dev;
  const mdr_snap* snap; const mdr_snap_halo* shalo; int row0;  // optional: snapshot (and ring halo) row row0 + t
  double* stats; int64_t stats_rows, stats_row0;               // optional: stats row stats_row0 + t
  uint8_t* act_row(int t, uint8_t* fallback) const { return action ? action + (int64_t)t * act_stride : fallback; }
  float* prob_row(int t) const { return prob ? prob + (int64_t)t * prob_stride : nullptr; }
  double* rew_row(int t) const { return reward + (int64_t)t * rew_stride; }
  double* stats_row(int t) const { return stats + (stats_row0 + t) * kTickRow; }
};

// Everything a captured actor rollout bakes into its launches (the head is, its epsilon is not: the kernels
// load it).  a.row0 is zero without a snapshot (it is ignored then), a.stats_row0 without stats rows; snap: the
// caller's by value, zero without one.  A call with a snapshot or stats rows never shares a graph with one without.
struct ActorGraphKey {
  ActorRolloutArgs a;
  mdr_snap snap;
  const void *comm_table, *halo_msg, *weights; int n_feat, head;  // (weights: the packed image)
  auto fields() const {
    return std::tie(a.n, a.action, a.act_stride, a.prob, a.prob_stride, a.reward, a.rew_stride, a.p_dev, comm_table,
                    halo_msg, n_feat, head, weights, snap.t_air, snap.t_mass, snap.hvac, snap.scalars, snap.row_stride,
                    a.row0, a.stats, a.stats_row0);
  }
  bool operator<(const ActorGraphKey& o) const { return fields() < o.fields(); }
};

}  // namespace

struct mdr_ctx {
  mdr_config cfg{};
  KParams kp{};
  bool bound = false;
  Dev<double> d_tables;                 // q_on[MDR_MAX_CAP] | p_on[MDR_MAX_CAP]
  Dev<unsigned long long> d_slab;        // kSlabs x kCountShards x n_cap count slabs (ring of 3 on
                                         // the step path, 4 in the overlapped sharded pipeline)
  int slab_len = 0;
  Validity v;                            // what the host believes the buffers hold (mdr_validity.h)
  Dev<double> d_pen_partial;             // 2 per block of k_step_t
  Dev<double> d_partial2;
  Dev<double> d_wpen;                    // common-penalty windows: {sum pen/N, max pen} [kWindowMax][tiles_padded][2]
  Dev<double> d_wres;                    // their per-tick {sum, max} [kWindowMax][2], then signal terms [kWindowMax]
  Dev<double> d_wstat;                   // closed-loop windows with stats rows: block partials [kWindowMax][grid][kStats]
  Dev<double> d_stat_p;                  // mdr_rollout_stats per tick without a caller's p_out: the tick's P
  Dev<double> d_ret_w;                   // mdr_rollout_returns: the call's staged weights (whole 32-byte records)
  Dev<double> d_ret_row;                 //   its scratch row [n_local]: the closed-loop windows' a_i, or the tick's rewards
  int pen_blocks = 0;
  // ---- options (mdr_set_option; defaults are the measured-fastest exact configuration)
  int tpw = 0;                           // MDR_OPT_STEP_TPW: k_step_pipe tiles per wave (0: k_step_t)
  bool fastdiv = true;                   // MDR_OPT_FASTDIV: shared-reciprocal exact division
  bool win_pipe = true;                  // MDR_OPT_WINDOW_PIPELINE: sharded count-ahead window pipeline
  bool tick_overlap = true;              // MDR_OPT_SHARDED_OVERLAP: per-tick sharded two-stream pipeline
  bool greedy_sort = false;              // MDR_OPT_GREEDY_SORT: the full-sort greedy form only
  bool force_halo = false;               // MDR_OPT_FORCE_HALO: sharded actor halo exchange at world 1
  bool actor_generic = false;            // MDR_OPT_ACTOR_GENERIC: no default-layout k_actor form
  int actor_grid = 0;                    // MDR_OPT_ACTOR_GRID: cap of k_actor's grid in blocks (0: n_cu)
  bool actor_fp32_bf16 = false;          // MDR_OPT_ACTOR_FP32_FORM: the three-way bf16 fp32 form (kernel PREC 6)
  bool halo_overlap = true;              // MDR_OPT_HALO_OVERLAP: sharded actor tick, halo beside the interior tiles
  bool halo_in_counts = true;            // MDR_OPT_HALO_IN_COUNTS: the next tick's ring halo rides in the count allreduce
  Dev<unsigned long long> d_c5;          // that path's ring of 3 x [count slab | world x halo rows]
  int thermal = MDR_THERMAL_AFFINE;      // MDR_OPT_WINDOW_THERMAL: k_step_window's per-tick update
  int win = kWindowMax;                  // ticks per k_step_window launch (0: one-tick path)
  Dev<unsigned long long> d_wslab;       // kWinSlots window count slots (mdr_kernels.hip K1W: slab | red | rec)
  int wslab_len = 0;
  Dev<uint64_t> d_onb;                   // per-tick ON lane masks of the next window [tiles][kWindowMax][HPT],
                                         // then (from onb_rows on) two halves of group rows
                                         // [tiles][kWinGroup][kWindowMax][HPT] (group_rows: a launch reads one, writes the other)
  size_t onb_rows = 0;                   // u64 words of the first part (the whole buffer before window groups)
  int win_group = kWinGroup;             // MDR_OPT_WINDOW_GROUP: windows per k_step_group launch (0: k_step_window)
  bool carry = true;                     // MDR_OPT_ROLLOUT_CARRY: a call's last step launch counts the next call's first group
  int la_order = MDR_LA_ALT8 | MDR_LA_TAIL_BEFORE;  // MDR_OPT_GROUP_LA_ORDER: which blocks of a k_step_group launch count
                                         // before they step (the measured default)
  std::map<const void*, int> grp_resident;  // resident blocks of a k_step_group instantiation (occupancy API x CUs)
  Dev<uint32_t> d_wah;                   // FSM word at the end of the next window, per house
  Dev<uint64_t> d_onb2;                  // second set for the count-ahead pipeline (pipe_buffers: a unit)
  Dev<uint32_t> d_wah2;
  Dev<int> d_flags;                      // [0] params_bad
  Dev<unsigned> d_tickets;               // k_count_window's grid_last_block counters (zero between uses)
  // rollout tick drivers (a unit with d_obs_sc: ensure_ticks)
  Dev<TickArgs> d_ticks;
  std::map<GraphKey, std::pair<hipGraphExec_t, int>> graphs;  // exec, the ring at the end of its capture
  // greedy scratch: one unit (greedy_scratch / greedy_clear), sized for g_cap houses
  int64_t g_cap = 0;
  Dev<double> g_key, g_key2, g_ps, g_incl;
  Dev<int> g_idx, g_idx2;
  Dev<uint8_t> g_ls;
  Dev<unsigned char> g_tmp;              // hipCUB's temporary storage (capacity in bytes)
  Dev<int64_t> g_kpos, g_extra;
  // histogram-select greedy (k_gq_*): partial min/max, bin histogram, selection, staged window
  Dev<double> g_part;
  Dev<unsigned> g_hist;
  Dev<unsigned char> g_sel_rec;          // the GqSel record's kGqSelBytes (the type is the kernels' own)
  GqSel* g_sel = nullptr;                //   and the kernels' view of it
  Dev<uint4> g_win;                      // the candidate window, unordered (k_gq_compact)
  Dev<uint32_t> g_map;                   // the key -> bin map's cells (gq_bin; k_gq_bins writes the next)
  Dev<unsigned> g_tickets;               // k_gq_select's grid_last_block counters
  Dev<double> g_range;                   // sharded select: this shard's (min, -max) key range (k_gq_range)
  Dev<uint4> g_sorted;                   // the window in (key, house) order (k_gq_select)
  int gq_parts_cap = 0;                  // g_part capacity in (min, max) pairs
  bool gq_band = true;                   // MDR_OPT_GQ_BAND: k_gq_binsc (the predicted band) vs k_gq_bins
  // the fused greedy tick (mdr_greedy_rollout; mdr_kernels.h GqfBufs)
  bool gq_adaptive = true;               // MDR_OPT_GQ_ADAPTIVE: mdr_greedy_rollout skips the band on budget jumps
  bool gq_band_skip = false;             // (set around one mdr_ctrl_greedy call by mdr_greedy_rollout)
  bool gq_fused = false;                 // MDR_OPT_GQ_FUSED (r06: slower than the band form)
  GqfBufs fz{};                          // views of the blocks below, as the kernels take them
  Dev<unsigned> fz_regions;              // par[0] | par[1] | miss
  Dev<uint4> fz_bkt, fz_mbkt;            // bkt[0] | bkt[1]; mbkt
  Dev<uint32_t> fz_maps;                 // map[0] | map[1]
  Dev<unsigned char> fz_sel;             // sel (kGqSelBytes)
  Dev<uint8_t> fz_dec;
  Dev<unsigned long long> fz_stamps;     // stamps: not of the unit (it survives a regrow)
  int64_t fz_cap_n = 0;                  // the cluster size the unit is allocated for (gqf_scratch / gqf_clear)
  // multi-GPU
  ncclComm_t comm = nullptr;
  struct {                               // mdr_comm_host: the caller's collectives instead of RCCL
    mdr_host_allreduce_fn allreduce = nullptr;
    mdr_host_sendrecv_fn sendrecv = nullptr;
    void* user = nullptr;
  } host;
  int world = 1, rank = 0;
  hipStream_t comm_stream = nullptr;     // per-tick / per-window allreduces of the overlapped pipelines
  hipStream_t cap_stream = nullptr;      // graph capture (graphs are replayed on the caller's stream)
  hipEvent_t ev_k1[kSlabs] = {}, ev_ar[kSlabs] = {}, ev_pc = nullptr;
  hipEvent_t ev[16] = {};
  std::vector<hipEvent_t>* step_events = nullptr;  // mdr_time_step_kernels: events around each step launch
  // MA-PPO actor (row P): packed weight image, per-tick obs scalars of actor rollouts
  Dev<unsigned char> d_actor;
  Dev<float> d_actor_raw;        // the loaded fp32 weights (w1 b1 w2 b2 w3 b3), packed per obs layout
  std::vector<int> actor_key;    // the slot layout + precision d_actor is packed for (empty: stale)
  mdr_actor_spec actor{};                // (the two-hidden-layer view the fused kernel packs from)
  mdr_actor_net net{};                   // the loaded actor: layers, widths, precision
  bool actor_ready = false;
  int actor_head = MDR_HEAD_SOFTMAX;     // mdr_actor_set_head: the output layer's head (in the actor graph keys)
  Dev<float> d_eps;                      // ... and the Q head's epsilon, read by every launch (never in a key)
  Dev<float> d_chain;                    // the chain's rows: obs [n][F] | hidden ping-pong 2 x [n][wmax4]
  int n_cu = 0;
  Dev<double> d_obs_sc;        // [d_ticks.capacity()][4]
  Dev<uint8_t> d_act;          // [n_local] actor actions when the caller keeps none
  Dev<float> d_halo;           // sharded actor rollout: packed edge rows | received ring halo
  Dev<double> d_stats;         // k_cluster_stats block partials
  Dev<double> d_tick_part;     // k_tick_stats block partials
  Dev<double> d_rows_part;     // mdr_greedy_rollout_stats: [kTickRowsBatch][kTickBlocks][kStats] block partials
  Dev<double> d_rows_p;        //   and the batch's [kTickRowsBatch] cluster powers
  Dev<double> d_xstat;         // sharded stats rows: the exchange slab X[world][m][kTickRow], all zero between calls
  int x_world = 0, x_rank = 0; // mdr_stats_exchange_ranks: the slab's world / rank on a shard without a communicator
  std::map<ActorGraphKey, std::pair<hipGraphExec_t, int>> actor_graphs;  // (as graphs)
  int64_t graph_launches[2] = {0, 0};  // hipGraphLaunch calls: rollout graphs, actor rollout graphs
  int64_t graphs_guarded = 0;            // captured graphs the memset guard walked (graph_memset_guard)
  int64_t graph_nodes_checked = 0;       //   and their nodes
  // a batch of independent clusters (mdr_batch_set): batch.n_envs != 0 is the mark
  BatchArgs batch{};
  Dev<uint64_t> d_batch_seeds;   // [n_envs] the clusters' Philox keys
  Dev<TickArgs> d_batch_ticks;   // [n_envs][n_ticks] of the call being issued (batch_reserve)
  Dev<double> d_batch_sc;        // [n_envs][4] mdr_batch_obs' scalars
  // interpolated base power (row a10): grid | table | capacities
  Dev<double> d_interp;
  InterpArgs interp{};
  bool interp_ready = false;
};

namespace {

// the context has a communicator (the library's RCCL one, or the caller's host collectives)
bool has_comm(const mdr_ctx* c) { return c->comm != nullptr || c->host.allreduce != nullptr; }

// bound, and ONE cluster: what every entry point that forms a cluster-level quantity over the whole
// context asks first (a batch of clusters has the mdr_batch_* entry points)
int cluster_ready(const mdr_ctx* c, const std::string& who) {
  if (!c->bound) return fail(MDR_ESTATE, who + ": context not bound");
  if (c->batch.n_envs)
    return fail(MDR_ESTATE, who + ": the context holds a batch of clusters (mdr_batch_set); use the mdr_batch_* entry points");
  return MDR_OK;
}

// in-place allreduce ordered on st (op: the mdr_rccl_allreduce dtype codes; 0 = 64-bit sum, which
// the unsigned count slabs use: the same bits for sums below 2^63)
int comm_allreduce(mdr_ctx* c, void* buf, size_t count, int op, hipStream_t st) {
  if (c->comm) {
    const ncclDataType_t t = op == 0 ? ncclInt64 : op == 3 ? ncclUint32 : ncclFloat64;
    const ncclRedOp_t o = op == 2 ? ncclMax : op == 4 ? ncclMin : ncclSum;
    RCCL_TRY(ncclAllReduce(buf, buf, count, t, o, c->comm, st));
    return MDR_OK;
  }
  if (!c->host.allreduce) return fail(MDR_ESTATE, "no communicator (mdr_rccl_init / mdr_comm_host)");
  HIP_TRY(hipStreamSynchronize(st));
  if (int r = c->host.allreduce(c->host.user, buf, (int64_t)count, op))
    return fail(MDR_ERCCL, "host allreduce callback failed (" + std::to_string(r) + ")");
  return MDR_OK;
}

// the 'neighbours' ring halo of a sharded obs: this shard's last lo rows (mine[hi, hi+lo)) to the
// next rank, its first hi rows to the previous one; recv = [lo rows of prev | hi rows of next]
int comm_halo(mdr_ctx* c, float* mine, float* recv, int lo, int hi, int M, hipStream_t st) {
  const int prev = (c->rank + c->world - 1) % c->world, next = (c->rank + 1) % c->world;
  if (c->comm) {
    RCCL_TRY(ncclGroupStart());
    if (lo) {
      RCCL_TRY(ncclSend(mine + (size_t)hi * M, (size_t)lo * M, ncclFloat32, next, c->comm, st));
      RCCL_TRY(ncclRecv(recv, (size_t)lo * M, ncclFloat32, prev, c->comm, st));
    }
    if (hi) {
      RCCL_TRY(ncclSend(mine, (size_t)hi * M, ncclFloat32, prev, c->comm, st));
      RCCL_TRY(ncclRecv(recv + (size_t)lo * M, (size_t)hi * M, ncclFloat32, next, c->comm, st));
    }
    RCCL_TRY(ncclGroupEnd());
    return MDR_OK;
  }
  if (!c->host.sendrecv) return fail(MDR_ESTATE, "no communicator for the ring halo");
  HIP_TRY(hipStreamSynchronize(st));
  const int64_t b = (int64_t)sizeof(float) * M;
  if (lo)
    if (int r = c->host.sendrecv(c->host.user, mine + (size_t)hi * M, lo * b, next, recv, lo * b, prev, 1))
      return fail(MDR_ERCCL, "host sendrecv callback failed (" + std::to_string(r) + ")");
  if (hi)
    if (int r = c->host.sendrecv(c->host.user, mine, hi * b, prev, recv + (size_t)lo * M, hi * b, next, 2))
      return fail(MDR_ERCCL, "host sendrecv callback failed (" + std::to_string(r) + ")");
  return MDR_OK;
}

unsigned long long* slab_at(mdr_ctx* c, int r) { return c->d_slab + (size_t)((r % 3 + 3) % 3) * c->slab_len; }

// All count slabs to zero with a kernel, never hipMemsetAsync: these launch sequences are captured
// into graphs (mdr_rollout, mdr_actor_rollout), and on ROCm 7.2 a captured memset node wrote
// non-zero words (host stack addresses, 0x7fff....) into the slabs on every replay after the
// first (profiles/r05b_graph_memset_bisect.log: the slab only the memset touches, with every other
// node of the graph removed in turn; tools/graph_memset_repro.hip), which the chained actor's
// rollout read as counts of ~1e14 W in its first two ticks
int zero_slabs(mdr_ctx* c, hipStream_t st) {
  hipLaunchKernelGGL(k_zero_u64, dim3(1), dim3(256), 0, st, c->d_slab, (int64_t)kSlabs * c->slab_len);
  LAUNCH_CHECK("k_zero_u64");
  return MDR_OK;
}

int check_mode(int m) {
  return m == MDR_ACT_BUFFER || m == MDR_ACT_RANDOM || m == MDR_ACT_ALWAYS_ON ||
         m == MDR_ACT_BANGBANG || m == MDR_ACT_DEADBAND_BANGBANG;
}

bool lookahead_ok(int m) { return m != MDR_ACT_BUFFER; }

TickArgs to_tick(const mdr_tick* t) { return TickArgs{t->t_od_prev, t->solar, t->s_prev, t->tick}; }

// k_step_pipe depth measured on MI355X (profiles/r01b_kbench_pipe.log): 2 tiles per wave up to
// ~1.5M houses per shard, 4 above
int default_tpw(int64_t n) { return n <= 1572864 ? 2 : 4; }

// phase 1 into `slab` (nullptr: the current slab)
int launch_counts(mdr_ctx* c, const uint8_t* action, int mode, uint64_t tick, const TickArgs* tkp,
                  hipStream_t st, unsigned long long* slab = nullptr) {
  static_assert(MDR_ACT_BANGBANG == kActBangBang && MDR_ACT_DEADBAND_BANGBANG == kActDeadband,
                "the kernels take the bang-bang sources by their public ids");
  hipLaunchKernelGGL(k_power_counts, dim3(blocks(c->kp.n, 256 * kPcHouses)), dim3(256), 0, st, c->kp, action, mode,
                     tick, tkp, slab ? slab : slab_at(c, c->v.ring()));
  LAUNCH_CHECK("k_power_counts");
  return MDR_OK;
}

// parameter-derived state (the fast-division range flag) after a change; called before any
// launch sequence is captured, so graphs never contain it
int refresh_if_dirty(mdr_ctx* c, hipStream_t st) {
  if (!c->v.coef_dirty()) return MDR_OK;
  HIP_TRY(hipMemsetAsync(c->d_flags, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_refresh, dim3(blocks(c->kp.n, 256)), dim3(256), 0, st, c->kp, c->d_flags);
  LAUNCH_CHECK("k_refresh");
  c->v.coef_refreshed();
  return MDR_OK;
}

int greedy_scratch(mdr_ctx* c, int64_t n);
int launch_gq_keys(mdr_ctx* c, hipStream_t st, unsigned long long* slab, bool local_map = true);
int gq_hist_produce(mdr_ctx* c, hipStream_t st);
// the histogram select's per-house codes (gq_code, 4 B) live in the sort form's key buffer
uint32_t* gq_codes(mdr_ctx* c) { return reinterpret_cast<uint32_t*>(c->g_key.get()); }

// k_step launch with explicit count slabs; reward_lag: the launch writes the previous tick's
// reward from `cur` (nullptr: none), see k_step_t

int launch_step_on(mdr_ctx* c, const uint8_t* action, int mode, TickArgs tk, const TickArgs* tkp,
                   double* reward, int lookahead, int ctrl, uint8_t* ctrl_out, double* p_out,
                   const unsigned long long* cur, unsigned long long* nxt, unsigned long long* zer,
                   int reward_lag, hipStream_t st) {
  if (int rc = refresh_if_dirty(c, st)) return rc;
  const KParams kp = c->kp;
  const bool gq = ctrl == MDR_CTRL_GREEDY_KEYS;
  if (gq) {
    if (int rc = greedy_scratch(c, kp.n)) return rc;
    ctrl = MDR_CTRL_NONE;
  }
#define MDR_LAUNCH_STEP(F, A, LA)                                                                     \
  hipLaunchKernelGGL((k_step_t<2, F, A, LA>), dim3(blocks(kp.n, 512)), dim3(256), 0, st, kp, action, mode, \
                     tk, tkp, cur, reward, ctrl, ctrl_out, p_out, lookahead, nxt, zer, c->d_pen_partial,    \
                     reward_lag)
  const bool hot_random = mode == MDR_ACT_RANDOM && lookahead == MDR_ACT_RANDOM;
  const bool hot_buffer = mode == MDR_ACT_BUFFER && lookahead == 0;
  // software-pipelined form of the two hot configurations (k_step_pipe): individual_L2, <= 4
  // capacity classes, no controller output, no reward lag, 2-byte aligned action rows
  const bool pipe_ok = c->tpw >= 1 && c->fastdiv && (hot_random || hot_buffer) &&
                       kp.penalty_mode == MDR_PEN_INDIVIDUAL_L2 && kp.n_cap <= kPipeMaxCap &&
                       ctrl == MDR_CTRL_NONE && !reward_lag && (!action || ((uintptr_t)action & 1u) == 0);
  if (pipe_ok) {
    int tpw = c->tpw >= 8 ? 8 : c->tpw >= 4 ? 4 : c->tpw >= 2 ? 2 : 1;
    if (hot_buffer) tpw = tpw >= 4 ? 4 : 2;  // the instantiated buffer variants
    // the greedy controller's keys in the epilogue (buffer actions: the C3 loop; blocks of
    // kStepGqWaves waves), when its partials buffer holds this grid
    const unsigned nbg = blocks(blocks(kp.n, 128), kStepGqWaves * tpw);
    const bool epi = gq && hot_buffer && (int)nbg <= c->gq_parts_cap;
    const int nwv = epi ? kStepGqWaves : 4;
    const unsigned nb = blocks(blocks(kp.n, 128), nwv * tpw);  // every tile covered: ceil(tiles / (waves x tpw))
    const dim3 grid(nb);
    GqOut go{};
    if (epi) {
      if (int rc = gq_hist_produce(c, st)) return rc;
      go = GqOut{nullptr, gq_codes(c), c->g_part, c->g_hist, c->g_sel, c->g_map};
    }
#define MDR_LAUNCH_PIPE(T, A, LA, G)                                                                     \
  hipLaunchKernelGGL((k_step_pipe<T, A, LA, G>), grid, dim3(64 * nwv), 0, st, kp, action, tk, tkp, cur, reward, \
                     p_out, nxt, zer, go, GqfBufs{}, 0)
    if (hot_random) {
      if (tpw == 8) MDR_LAUNCH_PIPE(8, MDR_ACT_RANDOM, MDR_ACT_RANDOM, 0);
      else if (tpw == 4) MDR_LAUNCH_PIPE(4, MDR_ACT_RANDOM, MDR_ACT_RANDOM, 0);
      else if (tpw == 2) MDR_LAUNCH_PIPE(2, MDR_ACT_RANDOM, MDR_ACT_RANDOM, 0);
      else MDR_LAUNCH_PIPE(1, MDR_ACT_RANDOM, MDR_ACT_RANDOM, 0);
    } else if (epi) {
      if (tpw >= 4) MDR_LAUNCH_PIPE(4, MDR_ACT_BUFFER, 0, 1);
      else MDR_LAUNCH_PIPE(2, MDR_ACT_BUFFER, 0, 1);
    } else {
      if (tpw >= 4) MDR_LAUNCH_PIPE(4, MDR_ACT_BUFFER, 0, 0);
      else MDR_LAUNCH_PIPE(2, MDR_ACT_BUFFER, 0, 0);
    }
#undef MDR_LAUNCH_PIPE
    LAUNCH_CHECK("k_step_pipe");
    // (a lookahead's counts are in nxt: k_gq_keys leaves them, mdr_ctrl_greedy zeroes the slab)
    if (gq && !epi) return launch_gq_keys(c, st, lookahead ? nullptr : nxt);
    if (epi) c->v.keys_from_epilogue((int)nb);
    return MDR_OK;
  }
  if (c->fastdiv) {
    if (hot_random) MDR_LAUNCH_STEP(true, MDR_ACT_RANDOM, MDR_ACT_RANDOM);
    else if (hot_buffer) MDR_LAUNCH_STEP(true, MDR_ACT_BUFFER, 0);
    else MDR_LAUNCH_STEP(true, -1, -1);
  } else {
    MDR_LAUNCH_STEP(false, -1, -1);
  }
#undef MDR_LAUNCH_STEP
  LAUNCH_CHECK("k_step");
  if (gq) return launch_gq_keys(c, st, lookahead ? nullptr : nxt);
  return MDR_OK;
}

int launch_step(mdr_ctx* c, const uint8_t* action, int mode, TickArgs tk, const TickArgs* tkp,
                double* reward, int lookahead, int ctrl, uint8_t* ctrl_out, double* p_out,
                hipStream_t st) {
  int rc = launch_step_on(c, action, mode, tk, tkp, reward, lookahead, ctrl, ctrl_out, p_out,
                          slab_at(c, c->v.ring()), slab_at(c, c->v.ring() + 1), slab_at(c, c->v.ring() + 2), 0, st);
  if (rc) return rc;
  c->v.step_issued(lookahead != 0, ctrl == MDR_CTRL_GREEDY_KEYS);
  return MDR_OK;
}

}  // namespace

extern "C" {

// An entry point that may write the house state or the count slabs is entered (c may be null: the
// checks follow).  An early first-window count (mdr_rollout_begin) is only valid for the mdr_rollout
// that follows it directly, so it is discarded too.
static void enter_writer(mdr_ctx* c) {
  if (!c) return;
  c->v.drop_early_count();
  c->v.state_may_change();
}

#ifndef MDR_SRC_HASH
#define MDR_SRC_HASH "unstamped0000000"
#endif
const char* mdr_build_id(void) { return "MDR_SRC_HASH:" MDR_SRC_HASH; }

int mdr_abi_version(void) { return MDR_ABI_VERSION; }

int mdr_abi_sizes(int64_t* out, int n) {
  const int64_t v[9] = {(int64_t)sizeof(mdr_config), (int64_t)sizeof(mdr_soa), (int64_t)sizeof(mdr_tick),
                        (int64_t)sizeof(mdr_pop_spec), (int64_t)sizeof(mdr_obs_spec),
                        (int64_t)sizeof(mdr_obs_scalars), (int64_t)sizeof(mdr_actor_spec),
                        (int64_t)sizeof(mdr_interp_spec), (int64_t)sizeof(mdr_actor_net)};
  int k = 0;
  for (; out && k < n && k < 9; ++k) out[k] = v[k];
  return k;
}

const char* mdr_last_error(void) { return g_err.c_str(); }

int mdr_rollout_carry_info(mdr_ctx* c, int64_t* out, int n) {
  if (!c || !out || n < 0) return fail(MDR_EARG, "mdr_rollout_carry_info: bad argument");
  const CarryCounters& k = c->v.carry_counters();
  const int64_t v[4] = {k.speculated, k.consumed, k.dropped, c->v.carry().on ? 1 : 0};
  int i = 0;
  for (; i < n && i < 4; ++i) out[i] = v[i];
  return i;
}

int mdr_graph_info(mdr_ctx* c, int64_t* out, int n) {
  if (!c || !out || n < 0) return fail(MDR_EARG, "mdr_graph_info: bad argument");
  const int64_t v[6] = {(int64_t)c->graphs.size(), (int64_t)c->actor_graphs.size(), c->graph_launches[0],
                        c->graph_launches[1], c->graphs_guarded, c->graph_nodes_checked};
  int k = 0;
  for (; k < n && k < 6; ++k) out[k] = v[k];
  return k;
}

// the parameters of a memset node captured in this library's context, against
// what was passed, and what its replays leave in the slabs.  Captures hipMemsetAsync(d_slab, 0, all
// slabs) exactly as the r04 rollouts did, outside capture_graph (whose guard refuses memset nodes).
// out[0..12] = {nodes, memset nodes, dst == d_slab, value, elementSize, width, height, pitch,
// bytes passed, non-zero 64-bit words after replay 1 (slabs pre-filled with 0xA5), after replay 2
// (re-filled), after replay 3 (not re-filled), non-zero words after a kernel (k_zero_u64) zeroing}
int mdr_graph_memset_probe(mdr_ctx* c, int64_t* out, int n, void* stream) {
  enter_writer(c);
  if (!c || !out || n < 13) return fail(MDR_EARG, "mdr_graph_memset_probe: need out[13]");
  Sequence seq(c->v, Sequence::kRollout);  // (the slabs are overwritten)
  for (int k = 0; k < n; ++k) out[k] = 0;
  hipStream_t st = S(stream);
  HIP_TRY(hipStreamSynchronize(st));
  if (!c->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
  const size_t bytes = (size_t)kSlabs * c->slab_len * sizeof(unsigned long long);
  const size_t words = bytes / 8;
  hipGraph_t g;
  HIP_TRY(hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal));
  hipError_t e = hipMemsetAsync(c->d_slab, 0, bytes, c->cap_stream);
  hipError_t e2 = hipStreamEndCapture(c->cap_stream, &g);
  if (e != hipSuccess || e2 != hipSuccess) return fail(MDR_EHIP, "memset probe: capture failed");
  size_t nn = 0;
  hipGraphGetNodes(g, nullptr, &nn);
  std::vector<hipGraphNode_t> nodes(nn);
  if (nn) hipGraphGetNodes(g, nodes.data(), &nn);
  out[0] = (int64_t)nn;
  for (size_t i = 0; i < nn; ++i) {
    hipGraphNodeType t;
    if (hipGraphNodeGetType(nodes[i], &t) != hipSuccess || t != hipGraphNodeTypeMemset) continue;
    out[1] += 1;
    hipMemsetParams mp{};
    if (hipGraphMemsetNodeGetParams(nodes[i], &mp) == hipSuccess) {
      out[2] = mp.dst == (void*)c->d_slab;
      out[3] = (int64_t)mp.value;
      out[4] = (int64_t)mp.elementSize;
      out[5] = (int64_t)mp.width;
      out[6] = (int64_t)mp.height;
      out[7] = (int64_t)mp.pitch;
    }
  }
  out[8] = (int64_t)bytes;
  hipGraphExec_t ex;
  e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  if (e != hipSuccess) return fail(MDR_EHIP, std::string("memset probe: instantiate: ") + hipGetErrorString(e));
  std::vector<unsigned long long> h(words);
  auto nonzero = [&](int64_t* o) -> int {
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipMemcpy(h.data(), c->d_slab, bytes, hipMemcpyDeviceToHost));
    int64_t z = 0;
    for (size_t i = 0; i < words; ++i) z += h[i] != 0ull;
    *o = z;
    return MDR_OK;
  };
  int rc = MDR_OK;
  for (int r = 0; r < 3 && !rc; ++r) {
    if (r < 2) {
      hipMemsetAsync(c->d_slab, 0xA5, bytes, st);
    }
    if (hipGraphLaunch(ex, st) != hipSuccess) rc = fail(MDR_EHIP, "memset probe: launch");
    else rc = nonzero(&out[9 + r]);
  }
  hipGraphExecDestroy(ex);
  if (rc) return rc;
  if ((rc = zero_slabs(c, st))) return rc;
  return seq.end(nonzero(&out[12]));
}

int mdr_create(mdr_ctx** out, const mdr_config* cfg) {
  if (!out || !cfg) return fail(MDR_EARG, "mdr_create: null argument");
  if (cfg->abi_version != MDR_ABI_VERSION) return fail(MDR_EARG, "mdr_create: ABI version mismatch");
  if (cfg->n_local < 1 || cfg->n_global < cfg->n_local || cfg->global_offset < 0 ||
      cfg->global_offset + cfg->n_local > cfg->n_global)
    return fail(MDR_EARG, "mdr_create: bad shard geometry");
  if (cfg->n_local >= ((int64_t)1 << 29))
    return fail(MDR_EARG, "mdr_create: n_local must be < 2^29 (32-bit byte offsets); shard across GPUs");
  if (cfg->n_cap < 1 || cfg->n_cap > MDR_MAX_CAP) return fail(MDR_EARG, "mdr_create: n_cap out of range");
  if (cfg->dt < 0) return fail(MDR_EARG, "mdr_create: negative dt");
  if (cfg->penalty_mode < 0 || cfg->penalty_mode > 3) return fail(MDR_EARG, "mdr_create: bad penalty mode");
  HIP_TRY(hipSetDevice(cfg->device));
  mdr_ctx* c = new mdr_ctx();
  c->cfg = *cfg;
  KParams& k = c->kp;
  k.n = cfg->n_local;
  k.goff = cfg->global_offset;
  k.n_global = cfg->n_global;
  k.dt = cfg->dt;
  k.L = cfg->lockout_duration;
  k.n_cap = cfg->n_cap;
  k.penalty_mode = cfg->penalty_mode;
  k.deadband = cfg->deadband;
  k.alpha_temp = cfg->alpha_temp;
  k.alpha_sig = cfg->alpha_sig;
  k.norm_temp = cfg->norm_temp;
  k.norm_sig = cfg->norm_sig;
  k.alpha_ind_l2 = cfg->alpha_ind_l2;
  k.alpha_common_l2 = cfg->alpha_common_l2;
  k.alpha_common_max = cfg->alpha_common_max;
  k.seed = cfg->seed;
  // capacity tables with the reference's expressions: hvac.py:94-97 and
  // environment_properties.py:92-98  (-1 * cap / (1 + lcf), cap / cop)
  double tab[2 * MDR_MAX_CAP] = {};
  for (int i = 0; i < cfg->n_cap; ++i) {
    tab[i] = (-1.0 * cfg->cap_table[i]) / (1.0 + cfg->lcf);
    tab[MDR_MAX_CAP + i] = cfg->cap_table[i] / cfg->cop;
  }
  auto cleanup = [&](int rc) { mdr_destroy(c); return rc; };
  if (c->d_tables.reserve(2 * MDR_MAX_CAP)) return cleanup(fail(MDR_ENOMEM, "tables"));
  if (hipMemcpy(c->d_tables, tab, sizeof(tab), hipMemcpyHostToDevice) != hipSuccess)
    return cleanup(fail(MDR_EHIP, "tables copy"));
  k.q_on = c->d_tables;
  k.p_on = c->d_tables + MDR_MAX_CAP;
  if (c->d_flags.reserve(4) || hipMemset(c->d_flags, 0, 16) != hipSuccess)
    return cleanup(fail(MDR_ENOMEM, "flags"));  // [0] params_bad, [1..2] the actor's fp16-range counts
  if (c->d_tickets.reserve(kTicketWords) ||
      hipMemset(c->d_tickets, 0, kTicketWords * sizeof(unsigned)) != hipSuccess)
    return cleanup(fail(MDR_ENOMEM, "tickets"));
  if (c->d_eps.reserve(1) || hipMemset(c->d_eps, 0, sizeof(float)) != hipSuccess)
    return cleanup(fail(MDR_ENOMEM, "epsilon"));
  k.params_bad = c->d_flags;
  {
    // the fast division is provably exact for dt < 2^20 s and |q_on| < 2^40 W (mdr_device.h)
    bool ok = cfg->dt < (1 << 20);
    for (int i = 0; i < cfg->n_cap; ++i) ok = ok && fabs(tab[i]) < kFastSolarAbs;
    k.fast_tick_ok = ok ? 1 : 0;
  }
  c->slab_len = kCountShards * cfg->n_cap;
  if (c->d_slab.reserve((size_t)kSlabs * c->slab_len))
    return cleanup(fail(MDR_ENOMEM, "count slabs"));
  if (hipMemset(c->d_slab, 0, kSlabs * c->slab_len * sizeof(unsigned long long)) != hipSuccess)
    return cleanup(fail(MDR_EHIP, "count slabs memset"));
  c->tpw = default_tpw(cfg->n_local);
  if (cfg->n_cap <= kWindowCap) {
    // a window count slot: sharded slab | reduced counts (mdr_kernels.hip)
    c->wslab_len = kWindowMax * kCountShards * cfg->n_cap + kWindowMax * cfg->n_cap + kWindowMax * kWindowRec;
    // 64-house lane groups of every wave tile a count / step-window grid launches: the grids round
    // the tiles up to whole blocks (up to kCountWaves tiles per block), and the waves of a ragged
    // last block store and load the mask rows of their (empty) tiles too
    const size_t tiles64 = whole_blocks(win_tiles(cfg->n_local) + 1, kCountWaves) * kWinHpt + 1;
    c->onb_rows = tiles64 * kWindowMax;
    if (c->d_wslab.reserve((size_t)kWinSlots * c->wslab_len) || c->d_onb.reserve((1 + 2 * kWinGroup) * c->onb_rows) ||
        c->d_wah.reserve((size_t)cfg->n_local + 1))
      return cleanup(fail(MDR_ENOMEM, "window count slabs"));
  } else {
    c->win = 0;
  }
  c->pen_blocks = (int)blocks(cfg->n_local, 512);  // = k_step_t grid
  if (c->d_pen_partial.reserve((size_t)2 * c->pen_blocks) || c->d_partial2.reserve(2))
    return cleanup(fail(MDR_ENOMEM, "penalty partials"));
  if (cfg->penalty_mode != MDR_PEN_INDIVIDUAL_L2 && c->d_wslab) {
    // windowed rollouts under a common penalty: the per-tick, per-wave partials (every wave of the
    // grid writes its rows each launch: never cleared) and the per-tick {sum, max} + signal term
    if (c->d_wpen.reserve(mdr_window_pen_bytes(cfg->n_local) / sizeof(double)) || c->d_wres.reserve(3 * kWindowMax))
      return cleanup(fail(MDR_ENOMEM, "window penalty partials"));
  }
  for (auto& e : c->ev)
    if (hipEventCreate(&e) != hipSuccess) return cleanup(fail(MDR_EHIP, "event"));
  for (int i = 0; i < kSlabs; ++i)
    if (hipEventCreateWithFlags(&c->ev_k1[i], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&c->ev_ar[i], hipEventDisableTiming) != hipSuccess)
      return cleanup(fail(MDR_EHIP, "event"));
  if (hipEventCreateWithFlags(&c->ev_pc, hipEventDisableTiming) != hipSuccess)
    return cleanup(fail(MDR_EHIP, "event"));
  if (hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device) != hipSuccess ||
      c->n_cu < 1)
    c->n_cu = 256;
  *out = c;
  return MDR_OK;
}

// Cached graphs hold the addresses of the buffers their launches were captured with: a site that
// frees such a buffer (d_ticks / d_obs_sc; d_actor, d_actor_raw, d_chain) drops them BEFORE it frees
static void drop_rollout_graphs(mdr_ctx* c) {
  for (auto& g : c->graphs) hipGraphExecDestroy(g.second.first);
  c->graphs.clear();
}

static void drop_actor_graphs(mdr_ctx* c) {
  for (auto& g : c->actor_graphs) hipGraphExecDestroy(g.second.first);
  c->actor_graphs.clear();
}

static void destroy_graphs(mdr_ctx* c) {
  drop_rollout_graphs(c);
  drop_actor_graphs(c);
}

// (the device buffers go with the context's destructor; mdr_create's cleanup comes here half-built)
int mdr_destroy(mdr_ctx* c) {
  if (!c) return MDR_OK;
  hipSetDevice(c->cfg.device);
  hipDeviceSynchronize();
  destroy_graphs(c);
  for (auto& e : c->ev)
    if (e) hipEventDestroy(e);
  for (int i = 0; i < kSlabs; ++i) {
    if (c->ev_k1[i]) hipEventDestroy(c->ev_k1[i]);
    if (c->ev_ar[i]) hipEventDestroy(c->ev_ar[i]);
  }
  if (c->ev_pc) hipEventDestroy(c->ev_pc);
  if (c->comm_stream) hipStreamDestroy(c->comm_stream);
  if (c->cap_stream) hipStreamDestroy(c->cap_stream);
  if (c->comm) ncclCommDestroy(c->comm);
  delete c;
  return MDR_OK;
}

int mdr_set_option(mdr_ctx* c, int option, int64_t value) {
  enter_writer(c);  // (writes no state; kept as it was: DESIGN §7.2, the sites kept for compatibility)
  if (!c) return fail(MDR_EARG, "mdr_set_option: null ctx");
  switch (option) {
    case MDR_OPT_STEP_TPW:
      if (value < -1 || value > 8) return fail(MDR_EARG, "mdr_set_option: STEP_TPW outside -1..8");
      c->tpw = value < 0 ? default_tpw(c->kp.n) : (int)value;
      break;
    case MDR_OPT_FASTDIV: c->fastdiv = value != 0; break;
    case MDR_OPT_WINDOW_PIPELINE: c->win_pipe = value != 0; break;
    case MDR_OPT_SHARDED_OVERLAP: c->tick_overlap = value != 0; break;
    case MDR_OPT_GREEDY_SORT: c->greedy_sort = value != 0; break;
    case MDR_OPT_FORCE_HALO: c->force_halo = value != 0; break;
    case MDR_OPT_HALO_OVERLAP: c->halo_overlap = value != 0; break;
    case MDR_OPT_HALO_IN_COUNTS: c->halo_in_counts = value != 0; break;
    case MDR_OPT_GQ_BAND: c->gq_band = value != 0; break;
    case MDR_OPT_GQ_FUSED:
      if (c->gq_fused != (value != 0)) c->v.map_form_switched();
      c->gq_fused = value != 0;
      break;
    case MDR_OPT_GQ_ADAPTIVE: c->gq_adaptive = value != 0; break;
    case MDR_OPT_ACTOR_GENERIC: c->actor_generic = value != 0; break;
    case MDR_OPT_ACTOR_GRID:
      if (value < 0) return fail(MDR_EARG, "mdr_set_option: ACTOR_GRID must be >= 0");
      c->actor_grid = (int)std::min<int64_t>(value, (int64_t)c->n_cu);  // (0: no cap)
      break;
    case MDR_OPT_ACTOR_FP32_FORM:
      if (value != MDR_FP32_F16_SPLIT && value != MDR_FP32_BF16_SPLIT3)
        return fail(MDR_EARG, "mdr_set_option: ACTOR_FP32_FORM must be MDR_FP32_F16_SPLIT or MDR_FP32_BF16_SPLIT3");
      c->actor_fp32_bf16 = value == MDR_FP32_BF16_SPLIT3;
      c->actor_key.clear();  // (packed again for the form)
      break;
    case MDR_OPT_WINDOW_GROUP:
      if (value < 0 || value > kWinGroup) return fail(MDR_EARG, "mdr_set_option: WINDOW_GROUP outside 0..4");
      c->win_group = (int)value;
      break;
    case MDR_OPT_WINDOW_THERMAL:
      if (value != MDR_THERMAL_EXACT && value != MDR_THERMAL_AFFINE)
        return fail(MDR_EARG, "mdr_set_option: WINDOW_THERMAL must be MDR_THERMAL_EXACT or _AFFINE");
      c->thermal = (int)value;
      break;
    case MDR_OPT_ROLLOUT_CARRY: c->carry = value != 0; break;
    case MDR_OPT_GROUP_LA_ORDER:
      if (value < 0 || value > INT32_MAX || (value & 0xf) > MDR_LA_BEFORE || (value & 0xe0))
        return fail(MDR_EARG, "mdr_set_option: GROUP_LA_ORDER: unknown pattern");
      c->la_order = (int)value;
      break;
    default: return fail(MDR_EARG, "mdr_set_option: unknown option");
  }
  HIP_TRY(hipDeviceSynchronize());  // cached graphs may be in flight
  destroy_graphs(c);
  return MDR_OK;
}

int mdr_bind(mdr_ctx* c, const mdr_soa* s) {
  enter_writer(c);
  if (!c || !s) return fail(MDR_EARG, "mdr_bind: null argument");
  if (!s->t_air || !s->t_mass || !s->hvac || !s->ua || !s->ca || !s->cm || !s->hm || !s->target ||
      !s->cap_idx)
    return fail(MDR_EARG, "mdr_bind: null array");
  KParams& k = c->kp;
  k.t_air = s->t_air;
  k.t_mass = s->t_mass;
  k.hvac = s->hvac;
  k.ua = s->ua;
  k.ca = s->ca;
  k.cm = s->cm;
  k.hm = s->hm;
  k.target = s->target;
  k.cap_idx = s->cap_idx;
  c->bound = true;
  c->v.state_replaced();
  drop_rollout_graphs(c);
  return MDR_OK;
}

int mdr_populate(mdr_ctx* c, const mdr_pop_spec* sp, void* stream) {
  enter_writer(c);
  if (!c || !sp) return fail(MDR_EARG, "mdr_populate: null argument");
  if (!c->bound) return fail(MDR_ESTATE, "mdr_populate: context not bound");
  if (sp->n_draw < 0 || sp->n_draw > MDR_MAX_CAP) return fail(MDR_EARG, "mdr_populate: n_draw out of range");
  for (int k = 0; k < sp->n_draw; ++k)
    if (sp->draw_idx[k] >= c->cfg.n_cap) return fail(MDR_EARG, "mdr_populate: draw_idx outside the cap table");
  PopArgs a{sp->target_temp, sp->std_target, sp->thermo_lo, sp->thermo_hi, sp->ca, sp->cm, sp->hm,
            sp->init_air, sp->init_mass, sp->n_draw, {}};
  memcpy(a.draw_idx, sp->draw_idx, sizeof(a.draw_idx));
  hipLaunchKernelGGL(k_populate, dim3(blocks(c->kp.n, 256)), dim3(256), 0, S(stream), c->kp, a);
  LAUNCH_CHECK("k_populate");
  c->v.state_replaced();
  return MDR_OK;
}

int mdr_power_counts(mdr_ctx* c, const uint8_t* action, int mode, uint64_t tick, void* stream) {
  enter_writer(c);
  if (!c) return fail(MDR_EARG, "mdr_power_counts: null ctx");
  if (int rc_ = cluster_ready(c, "mdr_power_counts")) return rc_;
  if (!check_mode(mode) || (mode == MDR_ACT_BUFFER && !action))
    return fail(MDR_EARG, "mdr_power_counts: bad action source");
  Sequence seq(c->v);
  // (re)compute this tick's counts from zero (a previous lookahead may have filled the slab)
  HIP_TRY(hipMemsetAsync(slab_at(c, c->v.ring()), 0, c->slab_len * sizeof(unsigned long long), S(stream)));
  int rc = launch_counts(c, action, mode, tick, nullptr, S(stream));
  if (rc) return rc;
  c->v.counts_produced();
  return seq.ok();
}

int mdr_counts_buffer(mdr_ctx* c, int64_t** ptr, int* len) {
  if (!c || !ptr || !len) return fail(MDR_EARG, "mdr_counts_buffer: null argument");
  *ptr = reinterpret_cast<int64_t*>(slab_at(c, c->v.ring()));
  *len = c->slab_len;
  return MDR_OK;
}

int mdr_step(mdr_ctx* c, const uint8_t* action, int mode, const mdr_tick* tick, double* reward,
             int lookahead, int ctrl, uint8_t* ctrl_out, double* p_out, void* stream) {
  enter_writer(c);
  if (!c || !tick || !reward) return fail(MDR_EARG, "mdr_step: null argument");
  if (int rc_ = cluster_ready(c, "mdr_step")) return rc_;
  if (!check_mode(mode) || (mode == MDR_ACT_BUFFER && !action))
    return fail(MDR_EARG, "mdr_step: bad action source");
  if (lookahead && (!check_mode(lookahead) || !lookahead_ok(lookahead)))
    return fail(MDR_EARG, "mdr_step: bad lookahead source");
  if (ctrl < MDR_CTRL_NONE || ctrl > MDR_CTRL_GREEDY_KEYS) return fail(MDR_EARG, "mdr_step: bad ctrl");
  if (!c->v.counts_ready()) return fail(MDR_ESTATE, "mdr_step: no cluster-power counts for this tick (call mdr_power_counts)");
  Sequence seq(c->v);
  return seq.end(launch_step(c, action, mode, to_tick(tick), nullptr, reward, lookahead, ctrl, ctrl_out, p_out,
                             S(stream)));
}

int mdr_penalty_partials(mdr_ctx* c, void* stream) {
  if (!c) return fail(MDR_EARG, "mdr_penalty_partials: null ctx");
  hipLaunchKernelGGL(k_pen_reduce, dim3(1), dim3(256), 0, S(stream), c->d_pen_partial, c->pen_blocks,
                     c->d_partial2);
  LAUNCH_CHECK("k_pen_reduce");
  return MDR_OK;
}

int mdr_penalty_buffer(mdr_ctx* c, double** ptr) {
  if (!c || !ptr) return fail(MDR_EARG, "mdr_penalty_buffer: null argument");
  *ptr = c->d_partial2;
  return MDR_OK;
}

int mdr_reward_finalize(mdr_ctx* c, const mdr_tick* tick, double* reward, void* stream) {
  if (!c || !tick || !reward) return fail(MDR_EARG, "mdr_reward_finalize: null argument");
  // the tick's counts are in the slab just before the current one
  hipLaunchKernelGGL(k_reward_finalize, dim3(blocks(c->kp.n, 256)), dim3(256), 0, S(stream), c->kp,
                     to_tick(tick), slab_at(c, c->v.ring() - 1), c->d_partial2, reward);
  LAUNCH_CHECK("k_reward_finalize");
  return MDR_OK;
}

// ------------------------------------------------------------------------------------ rollout
// n 32-byte records from host memory into device memory on `st`, through kernel arguments:
// nothing on the host waits for the device, and the host array may be reused on return
static int stage_recs(const void* src, int n, void* dst, hipStream_t st) {
  const Rec32* s = static_cast<const Rec32*>(src);
  Rec32* d = static_cast<Rec32*>(dst);
  for (int off = 0; off < n; off += kStageRecs) {
    const int m = n - off < kStageRecs ? n - off : kStageRecs;
    StagePack pk;
    memcpy(pk.r, s + off, (size_t)m * sizeof(Rec32));
    hipLaunchKernelGGL(k_stage32, dim3(1), dim3(kStageRecs), 0, st, pk, m, d + off);
    LAUNCH_CHECK("k_stage32");
  }
  return MDR_OK;
}

// the tick records and the actor rollouts' obs scalars: one unit, its capacity d_ticks'
static int ensure_ticks(mdr_ctx* c, int n) {
  if ((size_t)n <= c->d_ticks.capacity()) return MDR_OK;
  HIP_TRY(hipDeviceSynchronize());  // queued graphs may still read the old buffers
  destroy_graphs(c);                // (they hold the old addresses: gone before the buffers are)
  const size_t cap = n < 128 ? 128 : n;
  return grow_unit([&] { c->d_ticks.reset(), c->d_obs_sc.reset(); },
                   [&] {
                     if (int rc = dev_reserve(c->d_ticks, cap, "d_ticks")) return rc;
                     return dev_reserve(c->d_obs_sc, cap * 4, "d_obs_sc");
                   });
}

static int stage_ticks(mdr_ctx* c, int n, const mdr_tick* ticks, hipStream_t st) {
  if (int rc = ensure_ticks(c, n)) return rc;
  // stream order: every earlier launch reading d_ticks (a replayed graph) precedes this write
  return stage_recs(ticks, n, c->d_ticks, st);
}

// every node of a captured graph must be a kernel (the launch sequences hold nothing else); a memset
// node fails the capture with MDR_EHIP.  Counts the graphs checked (mdr_graph_info[4]).
static int graph_memset_guard(mdr_ctx* c, hipGraph_t g) {
  size_t nn = 0;
  HIP_TRY(hipGraphGetNodes(g, nullptr, &nn));
  std::vector<hipGraphNode_t> nodes(nn);
  if (nn) HIP_TRY(hipGraphGetNodes(g, nodes.data(), &nn));
  for (size_t i = 0; i < nn; ++i) {
    hipGraphNodeType t;
    HIP_TRY(hipGraphNodeGetType(nodes[i], &t));
    if (t == hipGraphNodeTypeMemset)
      return fail(MDR_EHIP, "capture: graph node " + std::to_string(i) + " of " + std::to_string(nn) +
                                " is a memset (captured launch sequences must zero with kernels)");
  }
  c->graphs_guarded += 1;
  c->graph_nodes_checked += (int64_t)nn;
  return MDR_OK;
}

// Capture a launch sequence into an executable graph on the context's own capture stream (the
// capture executes nothing), so the graph can then be launched on ANY caller stream — the null
// stream included — with no cross-stream synchronisation around each replay.
extern "C++" template <typename F>
static int capture_graph(mdr_ctx* c, F&& launches, hipGraphExec_t* out) {
  if (!c->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking));
  hipGraph_t g;
  HIP_TRY(hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeThreadLocal));
  const int rc = launches(c->cap_stream);
  hipError_t e = hipStreamEndCapture(c->cap_stream, &g);
  if (rc) return rc;
  if (e != hipSuccess) return fail(MDR_EHIP, std::string("capture: ") + hipGetErrorString(e));
  // memset guard: a captured hipMemsetAsync node left non-zero words in the count slabs on every
  // replay after the first (zero_slabs) — no captured graph may contain one
  if (int grc = graph_memset_guard(c, g)) {
    hipGraphDestroy(g);
    return grc;
  }
  e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
  hipGraphDestroy(g);
  if (e != hipSuccess) return fail(MDR_EHIP, std::string("instantiate: ") + hipGetErrorString(e));
  // upload the executable graph now (capture time), not on its first replay
  e = hipGraphUpload(*out, c->cap_stream);
  if (e != hipSuccess) return fail(MDR_EHIP, std::string("graph upload: ") + hipGetErrorString(e));
  return MDR_OK;
}

// The graph of `launches` cached under `key` (captured on first use, with the ring its capture ends
// on) replayed on st.  counter: its slot of graph_launches (mdr_graph_info).
extern "C++" template <class Map, class F>
static int replay_graph(mdr_ctx* c, Map& graphs, int counter, const typename Map::key_type& key, F&& launches,
                        hipStream_t st) {
  auto it = graphs.find(key);
  if (it == graphs.end()) {
    hipGraphExec_t ex;
    if (int rc = capture_graph(c, launches, &ex)) return rc;
    it = graphs.emplace(key, std::make_pair(ex, c->v.ring())).first;
  }
  HIP_TRY(hipGraphLaunch(it->second.first, st));
  ++c->graph_launches[counter];
  c->v.graph_replayed(it->second.second);
  return MDR_OK;
}

// ---- windowed rollout (k_step_window): open-loop action sources; the common penalty modes run
// its COMMON variant and two finish kernels per window (win_pen_finish), unsharded contexts only
// SIMPLE = deadband 0, norm_temp 1, and reward weights whose signal / temperature penalties are
// >= +0 (k_step_window forms -(a + s) as (-a) + (-s), exact for such operands)
static bool win_simple(const mdr_ctx* c) {
  return c->kp.deadband == 0.0 && c->kp.norm_temp == 1.0 && c->kp.alpha_temp >= 0.0 && !std::signbit(c->kp.alpha_temp) &&
         c->kp.alpha_sig >= 0.0 && !std::signbit(c->kp.alpha_sig) && c->kp.norm_sig > 0.0;
}

static bool win_common(const mdr_ctx* c) { return c->kp.penalty_mode != MDR_PEN_INDIVIDUAL_L2; }

// (the lookahead's FSM runs on unsaturated seconds-since-off in a signed offset form: L <= 2^30 - 1,
// dt <= 2^25, so a saturated value plus 33 ticks of dt and L - 32 dt stay inside int32 —
// mdr_kernels.hip win_run_t)
static bool window_geom_ok(const mdr_ctx* c) {
  return c->win > 0 && c->d_wslab && c->kp.n_cap <= kWindowCap && c->kp.L < (1 << 30) && c->kp.dt >= 0 &&
         c->kp.dt <= (1 << 25);
}

static bool window_ok(const mdr_ctx* c, int mode) {
  return window_geom_ok(c) && (win_common(c) ? c->d_wpen != nullptr : true) &&
         (mode == MDR_ACT_RANDOM || mode == MDR_ACT_ALWAYS_ON || mode == MDR_ACT_BUFFER);
}

// the closed-loop window (k_step_closed): the bang-bang sources, the same window, class and L / dt
// conditions; a common penalty mode needs its partial rows (d_wpen / d_wres) and gives no stats rows
// (no STATS x COMMON instantiation).  Everything else of theirs runs one launch per tick
static bool closed_ok(const mdr_ctx* c, int mode, bool stats = false) {
  return window_geom_ok(c) && (win_common(c) ? !stats && c->d_wpen && c->d_wres : true) &&
         (mode == MDR_ACT_BANGBANG || mode == MDR_ACT_DEADBAND_BANGBANG);
}

// the window slots' shard part is zero between rollouts (k_win_reduce zeroes what it reads);
// after allocation or a failed launch sequence it is cleared once, outside any graph
static int wslab_clean(mdr_ctx* c, hipStream_t st) {
  if (!c->v.slots_dirty() || !c->d_wslab) return MDR_OK;
  HIP_TRY(hipMemsetAsync(c->d_wslab, 0, kWinSlots * sizeof(unsigned long long) * c->wslab_len, st));
  c->v.slots_cleaned();
  return MDR_OK;
}

static unsigned win_grid(const mdr_ctx* c, int waves = 4) {  // a tile per wave
  return (unsigned)(whole_blocks(win_tiles(c->kp.n), waves) / waves);
}

extern "C" size_t mdr_window_onb_bytes(int64_t n_local, int waves) {
  if (n_local < 0 || waves < 1) return 0;
  return whole_blocks(win_tiles(n_local), waves) * kWinHpt * kWindowMax * sizeof(uint64_t);
}

extern "C" int mdr_window_geometry_check(int64_t n_local, size_t onb_bytes, size_t wah_bytes) {
  if (n_local < 1) return fail(MDR_EARG, "window launch: no houses");
  const size_t need = std::max(mdr_window_onb_bytes(n_local, kCountWaves), mdr_window_onb_bytes(n_local, 4));
  if (onb_bytes < need)
    return fail(MDR_EARG, "window launch: ON-mask rows of " + std::to_string(onb_bytes) + " B, the launch geometry touches " +
                              std::to_string(need) + " B");
  if (wah_bytes < (size_t)n_local * sizeof(uint32_t))
    return fail(MDR_EARG, "window launch: end-word buffer shorter than the shard");
  return MDR_OK;
}

// k_step_group: every wave of the grid (4 tiles per block) reads and stores `windows` windows of
// mask rows per tile, and one end word per house
extern "C" int mdr_window_group_check(int64_t n_local, int windows, size_t onb_bytes, size_t wah_bytes) {
  if (n_local < 1) return fail(MDR_EARG, "window group launch: no houses");
  if (windows < 1 || windows > kWinGroup) return fail(MDR_EARG, "window group launch: windows outside 1..4");
  const size_t need = (size_t)windows * mdr_window_onb_bytes(n_local, 4);
  if (onb_bytes < need)
    return fail(MDR_EARG, "window group launch: ON-mask rows of " + std::to_string(onb_bytes) +
                              " B, the launch geometry touches " + std::to_string(need) + " B");
  if (wah_bytes < (size_t)n_local * sizeof(uint32_t))
    return fail(MDR_EARG, "window group launch: end-word buffer shorter than the shard");
  return MDR_OK;
}

// the two halves of group rows, packed: half h starts h * kWinGroup * mdr_window_onb_bytes(n_local, 4)
// bytes into the group rows; a launch reads kWinGroup windows of one and writes kWinGroup of the other
extern "C" size_t mdr_window_group_half_bytes(int64_t n_local) {
  return (size_t)kWinGroup * mdr_window_onb_bytes(n_local, 4);
}

extern "C" int mdr_window_group_halves_check(int64_t n_local, size_t onb_bytes, size_t wah_bytes) {
  if (int rc = mdr_window_group_check(n_local, kWinGroup, onb_bytes, wah_bytes)) return rc;
  const size_t need = 2 * mdr_window_group_half_bytes(n_local);
  if (onb_bytes < need)
    return fail(MDR_EARG, "window group launch: ON-mask rows of " + std::to_string(onb_bytes) +
                              " B, the two halves of group rows take " + std::to_string(need) + " B");
  return MDR_OK;
}

extern "C" size_t mdr_window_pen_bytes(int64_t n_local) {
  if (n_local < 0) return 0;
  return whole_blocks(win_tiles(n_local), 4) * kWindowMax * 2 * sizeof(double);  // (step-window blocks hold 4 waves)
}

extern "C" int mdr_window_pen_check(int64_t n_local, size_t pen_bytes) {
  if (n_local < 1) return fail(MDR_EARG, "window launch: no houses for the penalty partial rows");
  const size_t need = mdr_window_pen_bytes(n_local);
  if (pen_bytes < need)
    return fail(MDR_EARG, "window launch: penalty partial rows of " + std::to_string(pen_bytes) +
                              " B, the launch geometry writes " + std::to_string(need) + " B");
  return MDR_OK;
}

// k_step_closed<..., STATS = true>: every block stores kStats doubles per tick of a window
extern "C" size_t mdr_window_stats_bytes(int64_t n_local) {
  if (n_local < 0) return 0;
  return whole_blocks(win_tiles(n_local), 4) / 4 * kWindowMax * kStats * sizeof(double);  // (a block holds 4 waves, a tile each)
}

extern "C" int mdr_window_stats_check(int64_t n_local, size_t bytes) {
  if (n_local < 1) return fail(MDR_EARG, "window launch: no houses for the stats partial rows");
  const size_t need = mdr_window_stats_bytes(n_local);
  if (bytes < need)
    return fail(MDR_EARG, "window launch: stats partial rows of " + std::to_string(bytes) +
                              " B, the launch geometry writes " + std::to_string(need) + " B");
  return MDR_OK;
}

// the finish of a common-penalty window of K ticks behind its k_step_window (stream order: the
// kernel boundary publishes the step kernel's partials): per-tick {sum, max}, then the reward rows.
// One shared row (rew_stride == 0): only the window's last tick is finalised.
static int win_pen_finish(mdr_ctx* c, int K, double* reward, int64_t rew_stride, hipStream_t st) {
  const int ntile = (int)whole_blocks(win_tiles(c->kp.n), 4);
  double *res = c->d_wres, *sig = c->d_wres + 2 * kWindowMax;
  const int j0 = rew_stride ? 0 : K - 1;
  hipLaunchKernelGGL(k_win_pen_reduce, dim3(K - j0), dim3(256), 0, st,
                     (const double*)c->d_wpen + (size_t)j0 * ntile * 2, ntile, res + 2 * j0);
  LAUNCH_CHECK("k_win_pen_reduce");
  hipLaunchKernelGGL(k_win_reward_common, dim3(blocks(c->kp.n, 256), K - j0), dim3(256), 0, st, c->kp,
                     (const double*)res, (const double*)sig, j0, reward, rew_stride);
  LAUNCH_CHECK("k_win_reward_common");
  return MDR_OK;
}

// the reduced per-tick class counts of a window slot (after its kWindowMax x 64 x n_cap shards)
static unsigned long long* win_red_ptr(const mdr_ctx* c, unsigned long long* slot) {
  return slot + (size_t)kWindowMax * kCountShards * c->kp.n_cap;
}

// a new event pair for one step launch while mdr_time_step_kernels measures (else null events)
static int step_event_pair(mdr_ctx* c, hipEvent_t* e0, hipEvent_t* e1) {
  *e0 = *e1 = nullptr;
  if (!c->step_events) return MDR_OK;
  HIP_TRY(hipEventCreate(e0));
  c->step_events->push_back(*e0);
  HIP_TRY(hipEventCreate(e1));
  c->step_events->push_back(*e1);
  return MDR_OK;
}

// a window's FSM count: ticks from tk (staged) or tick0 + j (tk == nullptr), from the
// state's FSM words (w_in == nullptr) or from the end words of the previous window
// p_only: the count kernel's last block also does the window's P-only reduce (win_reduce_last),
// for a first window whose drivers ride on the step launch and whose shards need no allreduce
static int launch_count(mdr_ctx* c, int mode, const uint8_t* action, int64_t act_stride, const TickArgs* tk,
                        uint64_t tick0, int K, unsigned long long* slot, uint64_t* onb, uint32_t* wah,
                        const uint32_t* w_in, hipStream_t st, bool p_only) {
  if (int rc = mdr_window_geometry_check(c->kp.n, dev_bytes(c->d_onb), dev_bytes(c->d_wah))) return rc;
  const unsigned grid = win_grid(c, kCountWaves);
  unsigned* ticket = p_only ? c->d_tickets : nullptr;
#define MDR_COUNT(A)                                                                                  \
  hipLaunchKernelGGL((k_count_window<A, kWinHpt>), dim3(grid), dim3(64 * kCountWaves), 0, st, c->kp, action, act_stride, tk, \
                     tick0, K, slot, onb, wah, w_in, ticket)
  if (mode == MDR_ACT_RANDOM) MDR_COUNT(MDR_ACT_RANDOM);
  else if (mode == MDR_ACT_ALWAYS_ON) MDR_COUNT(MDR_ACT_ALWAYS_ON);
  else MDR_COUNT(MDR_ACT_BUFFER);
#undef MDR_COUNT
  LAUNCH_CHECK("k_count_window");
  return MDR_OK;
}

// one k_step_window launch: the (ACT, SIMPLE, KA, FORM) instantiation for this context; with
// step_events (mdr_time_step_kernels) hipExtLaunchKernel's start / stop events time it
static int launch_step_window(mdr_ctx* c, int mode, bool ka, const uint8_t* action, int64_t act_stride,
                              const TickArgs* tk, int K, int la_K, const double* rec, double* reward,
                              int64_t rew_stride, uint64_t* onb, uint32_t* wah, unsigned long long* next_slot,
                              const WinDrv& dv, hipStream_t st) {
  if (int rc = mdr_window_geometry_check(c->kp.n, dev_bytes(c->d_onb), dev_bytes(c->d_wah))) return rc;
  const unsigned grid = win_grid(c);
  hipEvent_t t0, t1;
  if (int rc = step_event_pair(c, &t0, &t1)) return rc;
  const KParams kp = c->kp;
  // the common penalty modes: the COMMON variant (SIMPLE = false), its partial rows checked first
  const bool common = win_common(c);
  WinPen wp{};
  if (common) {
    if (!c->d_wpen || !c->d_wres) return fail(MDR_ESTATE, "window launch: no penalty partial rows");
    if (int rc = mdr_window_pen_check(c->kp.n, dev_bytes(c->d_wpen))) return rc;
    wp = WinPen{c->d_wpen, c->d_wres + 2 * kWindowMax};
  }
#define MDR_SW_L(A, SI, KA_, FO, CO)                                                                      \
  do {                                                                                                    \
    if (t0)                                                                                               \
      hipExtLaunchKernelGGL((k_step_window<A, kWinHpt, SI, KA_, FO, CO>), dim3(grid), dim3(256), 0, st, t0, t1, 0, kp, \
                            action, act_stride, tk, K, la_K, rec, reward, rew_stride, onb, wah, next_slot, dv, wp); \
    else                                                                                                  \
      hipLaunchKernelGGL((k_step_window<A, kWinHpt, SI, KA_, FO, CO>), dim3(grid), dim3(256), 0, st, kp, action, \
                         act_stride, tk, K, la_K, rec, reward, rew_stride, onb, wah, next_slot, dv, wp);   \
  } while (0)
#define MDR_SW_F(A, SI, KA_, CO)                                                            \
  do {                                                                                      \
    if (c->thermal == MDR_THERMAL_AFFINE) MDR_SW_L(A, SI, KA_, MDR_THERMAL_AFFINE, CO);     \
    else MDR_SW_L(A, SI, KA_, MDR_THERMAL_EXACT, CO);                                       \
  } while (0)
#define MDR_SW_K(A, SI, CO)                     \
  do {                                          \
    if (ka) MDR_SW_F(A, SI, true, CO);          \
    else MDR_SW_F(A, SI, false, CO);            \
  } while (0)
#define MDR_SW_S(A)                                  \
  do {                                               \
    if (common) MDR_SW_K(A, false, true);            \
    else if (win_simple(c)) MDR_SW_K(A, true, false); \
    else MDR_SW_K(A, false, false);                  \
  } while (0)
  if (mode == MDR_ACT_RANDOM) MDR_SW_S(MDR_ACT_RANDOM);
  else if (mode == MDR_ACT_ALWAYS_ON) MDR_SW_S(MDR_ACT_ALWAYS_ON);
  else MDR_SW_S(MDR_ACT_BUFFER);
#undef MDR_SW_S
#undef MDR_SW_K
#undef MDR_SW_F
#undef MDR_SW_L
  LAUNCH_CHECK("k_step_window");
  return MDR_OK;
}

// one k_step_group launch: the (ACT, SIMPLE, KA, FORM) instantiation for this context (individual_L2)
// wts (mdr_rollout_returns): k_step_group_ret instead, `reward` the returns row, wts the staged weights
// at the group's first tick
static int launch_step_group(mdr_ctx* c, int mode, bool ka, const uint8_t* action, int64_t act_stride,
                             const TickArgs* tk, const WinGrp& g_in, int wr_half, double* reward, int64_t rew_stride,
                             const WinDrv& dv, hipStream_t st, const double* wts = nullptr) {
  WinGrp g = g_in;
  if (c->d_onb.capacity() < c->onb_rows) return fail(MDR_ESTATE, "window group launch: no group mask rows");
  if (int rc = mdr_window_group_halves_check(c->kp.n, dev_bytes(c->d_onb) - c->onb_rows * sizeof(uint64_t),
                                             dev_bytes(c->d_wah)))
    return rc;
  if (wr_half != 0 && wr_half != 1) return fail(MDR_EARG, "window group launch: half outside 0..1");
  if (g.nw < 1 || g.nw > kWinGroup || g.la_nw < 0 || g.la_nw > kWinGroup)
    return fail(MDR_EARG, "window group launch: windows outside 1..4");
  for (int i = 0; i < kWinGroup; ++i)
    if (g.K[i] < 0 || g.K[i] > kWindowMax || g.la_K[i] < 0 || g.la_K[i] > kWindowMax)
      return fail(MDR_EARG, "window group launch: a window of more than 32 ticks");
  const unsigned grid = win_grid(c);
  const KParams kp = c->kp;
  // the group rows, behind the first window's: the lookahead writes half wr_half, the stepped windows'
  // rows are in the other (KA: the count kernel's rows, in front)
  uint64_t* const halves = c->d_onb + c->onb_rows;
  const size_t half_words = mdr_window_group_half_bytes(c->kp.n) / sizeof(uint64_t);
  uint64_t* onb = halves + (size_t)wr_half * half_words;
  g.rd_onb = ka ? c->d_onb.get() : halves + (size_t)(1 - wr_half) * half_words;
  // which blocks count before they step (MDR_OPT_GROUP_LA_ORDER)
  static const unsigned kShift[] = {31u, 0u, 3u, 8u, 31u};
  const int pat = c->la_order & 0xf;
  g.la_shift = kShift[pat];
  g.la_from = pat == MDR_LA_BEFORE ? 0u : UINT32_MAX;
  auto tail_from = [&](const void* fn) {  // the blocks past the first resident round go early
    if (ka || wts || c->thermal != MDR_THERMAL_AFFINE) return;  // (forms compiled with the one order: mdr_kernels.hip)
    if (c->la_order >> 8) { g.la_from = (unsigned)(c->la_order >> 8); return; }  // (the tests' threshold)
    if (!(c->la_order & MDR_LA_TAIL_BEFORE)) return;
    auto it = c->grp_resident.find(fn);
    if (it == c->grp_resident.end()) {
      int per_cu = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 256, 0) != hipSuccess || per_cu < 1) per_cu = 0;
      it = c->grp_resident.emplace(fn, per_cu * c->n_cu).first;
    }
    if (it->second > 0) g.la_from = (unsigned)it->second;
  };
#define MDR_SG_L(A, SI, KA_, FO)                                                                               \
  do {                                                                                                         \
    tail_from(wts ? (const void*)k_step_group_ret<A, kWinHpt, SI, KA_, FO> : (const void*)k_step_group<A, kWinHpt, SI, KA_, FO>); \
    if (wts)                                                                                                   \
      hipLaunchKernelGGL((k_step_group_ret<A, kWinHpt, SI, KA_, FO>), dim3(grid), dim3(256), 0, st, kp, action, \
                         act_stride, tk, g, reward, wts, onb, (uint32_t*)c->d_wah, c->d_wslab.get(), dv);                        \
    else                                                                                                       \
      hipLaunchKernelGGL((k_step_group<A, kWinHpt, SI, KA_, FO>), dim3(grid), dim3(256), 0, st, kp, action, act_stride, \
                         tk, g, reward, rew_stride, onb, (uint32_t*)c->d_wah, c->d_wslab.get(), dv);                             \
  } while (0)
#define MDR_SG_F(A, SI, KA_)                                                         \
  do {                                                                               \
    if (c->thermal == MDR_THERMAL_AFFINE) MDR_SG_L(A, SI, KA_, MDR_THERMAL_AFFINE);  \
    else MDR_SG_L(A, SI, KA_, MDR_THERMAL_EXACT);                                    \
  } while (0)
#define MDR_SG_K(A, SI)              \
  do {                               \
    if (ka) MDR_SG_F(A, SI, true);   \
    else MDR_SG_F(A, SI, false);     \
  } while (0)
#define MDR_SG_S(A)                          \
  do {                                       \
    if (win_simple(c)) MDR_SG_K(A, true);    \
    else MDR_SG_K(A, false);                 \
  } while (0)
  if (mode == MDR_ACT_RANDOM) MDR_SG_S(MDR_ACT_RANDOM);
  else if (mode == MDR_ACT_ALWAYS_ON) MDR_SG_S(MDR_ACT_ALWAYS_ON);
  else MDR_SG_S(MDR_ACT_BUFFER);
#undef MDR_SG_S
#undef MDR_SG_K
#undef MDR_SG_F
#undef MDR_SG_L
  LAUNCH_CHECK("k_step_group");
  return MDR_OK;
}

// ---- the open-loop window sequencers (window_launches, window_launches_direct,
// window_pipeline).  Window w of the WinPlan counts into slot w % 3 of d_wslab, under a SlotsGuard.
struct WinSeq {  // the per-window pieces the three share
  mdr_ctx* c;
  const RolloutArgs& a;
  hipStream_t st;
  WinPlan plan;
  const TickArgs* tk(int w) const { return c->d_ticks + plan.start(w); }
  unsigned long long* slot(int w) const { return c->d_wslab + (size_t)(w % 3) * c->wslab_len; }
  const double* rec(int w) const {  // the slot's tick records, after its shards and reduced counts
    return reinterpret_cast<const double*>(win_red_ptr(c, slot(w)) + (size_t)kWindowMax * c->kp.n_cap);
  }
  double* p_out(int w) const { return w == plan.count() - 1 ? a.p_out : nullptr; }  // the rollout's last P
  // window w's k_step_window, counting la ticks ahead into `next`; ka: the drivers as its arguments
  int step(int w, int la, uint64_t* onb, uint32_t* wah, unsigned long long* next, const WinDrv* ka = nullptr) const {
    static const WinDrv none{};
    const int t0 = plan.start(w);
    return launch_step_window(c, a.mode, ka != nullptr, a.act_row(t0), a.act_stride, tk(w), plan.size(w), la, rec(w),
                              a.rew_row(t0), a.rew_stride, onb, wah, next, ka ? *ka : none, st);
  }
  // the common penalty modes' finish, unless a later window overwrites the one shared row
  int finish(int w) const {
    if (!win_common(c) || (!a.rew_stride && w + 1 < plan.count())) return MDR_OK;
    return win_pen_finish(c, plan.size(w), a.rew_row(plan.start(w)), a.rew_stride, st);
  }
  // windows w0.. with staged drivers, each counted by its predecessor: k_win_reduce (shard sums ->
  // counts + tick records) -> k_step_window -> finish.  shd: the ranks' count shards (exact
  // integers, K x 64 x n_cap) are allreduced first, so the one reduce kernel yields global counts
  int staged_windows(int w0, bool shd) const {
    const int nw = plan.count(), ncap = c->kp.n_cap;
    for (int w = w0; w < nw; ++w) {
      const int K = plan.size(w);
      if (shd)
        if (int rc = comm_allreduce(c, slot(w), (size_t)K * kCountShards * ncap, 0, st)) return rc;
      hipLaunchKernelGGL(k_win_reduce, dim3(K), dim3(64 * ncap), 0, st, c->kp, slot(w), K, tk(w), p_out(w));
      LAUNCH_CHECK("k_win_reduce");
      if (int rc = step(w, w + 1 < nw ? plan.size(w + 1) : 0, c->d_onb, c->d_wah, slot(w + 1))) return rc;
      if (int rc = finish(w)) return rc;
    }
    return MDR_OK;
  }
};

// (a sharded sequence would have to allreduce the cluster's per-tick mean / max penalty)
static int win_common_unsharded(const mdr_ctx* c, bool shd) {
  if (!win_common(c) || !shd) return MDR_OK;
  return fail(MDR_EARG, "window launches: common penalty modes on a sharded context need the per-step API");
}

// The staged sequence: k_count_window for the first window, then staged_windows.  Tick drivers come
// from d_ticks for every window.  Kernels only (unsharded), so a graph may capture it.
static int window_launches(mdr_ctx* c, const RolloutArgs& a, bool shd, hipStream_t st) {
  if (int rc = win_common_unsharded(c, shd)) return rc;
  const WinSeq s{c, a, st, WinPlan(a.n, c->win)};
  SlotsGuard slots(c->v);  // dirty until the sequence is fully issued
  if (int rc = launch_count(c, a.mode, a.action, a.act_stride, c->d_ticks, 0, s.plan.size(0), s.slot(0), c->d_onb,
                            c->d_wah, nullptr, st, false))
    return rc;
  if (int rc = s.staged_windows(0, shd)) return rc;
  return slots.done();
}

// The direct sequence's windows in groups of G <= kWinGroup (MDR_OPT_WINDOW_GROUP): behind
// the first window's count, k_step_group<KA>({w0}; counting w1..wG ahead), the later drivers' staging,
// then per group one reduce launch and one k_step_group (counting the next group ahead).  Window w
// counts into slot w % kWinSlots.
// wts (mdr_rollout_returns): the call's staged weights; a.reward is then the returns row (stride 0)
// The call boundary (mdr_validity.h CarriedCount): with cb.speculate the call's LAST launch runs its
// lookahead on over the first min(G, nw) windows of the next call — the same plan from the id behind
// this call's last, into the slots behind this call's (carry_slot) — and with cb.carried this call's
// first group was counted that way: no count kernel and no KA launch, every driver staged, window 0
// in a staged group like any later one.  Window w counts into slot carry_slot(cb.slot_base, w).
struct CallBoundary {
  bool carried = false, speculate = false;
  int slot_base = 0;
  int half = 0;  // carried: the half of the group mask rows that holds the carried group (mdr_validity.h group_half)
};
static_assert(kCarryGroup == kWinGroup && kCarrySlots == kWinSlots, "mdr_validity.h mirrors the group geometry");
static int window_groups(const WinSeq& s, int G, const WinDrv& dv, const mdr_tick* host_ticks,
                         const double* wts = nullptr, const CallBoundary& cb = CallBoundary{}) {
  mdr_ctx* c = s.c;
  const RolloutArgs& a = s.a;
  const int nw = s.plan.count(), K0 = s.plan.size(0), ncap = c->kp.n_cap;
  auto slot = [&](int w) { return c->d_wslab + (size_t)carry_slot(cb.slot_base, w) * c->wslab_len; };
  auto rec = [&](int w) {
    return reinterpret_cast<const double*>(win_red_ptr(c, slot(w)) + (size_t)kWindowMax * ncap);
  };
  // the lookahead over the group that starts at window w1; w1 == nw: the next call's first group
  auto ahead = [&](WinGrp& g, int w1) {
    const bool next_call = w1 >= nw;
    g.la_nw = next_call ? (cb.speculate ? std::min(G, nw) : 0) : std::min(G, nw - w1);
    for (int i = 0; i < g.la_nw; ++i) g.la_K[i] = s.plan.size(next_call ? i : w1 + i), g.la_slot[i] = (size_t)(slot(w1 + i) - c->d_wslab.get());
    g.la_tick0 = host_ticks[0].tick + (uint64_t)(next_call ? a.n : s.plan.start(w1));
    g.la_by_id = next_call;  // (those ticks are not staged)
  };
  static const WinDrv none{};
  if (!cb.carried) {
    WinGrp g{};
    g.nw = 1, g.K[0] = K0, g.rec[0] = rec(0);
    ahead(g, 1);
    if (int rc = launch_step_group(c, a.mode, true, a.act_row(0), a.act_stride, s.tk(0), g, 0, a.rew_row(0), a.rew_stride,
                                   dv, s.st, wts))
      return rc;
    if (a.n > K0)
      if (int rc = stage_recs(host_ticks + K0, a.n - K0, c->d_ticks + K0, s.st)) return rc;
  } else if (int rc = stage_recs(host_ticks, a.n, c->d_ticks, s.st)) {
    return rc;
  }
  int k = 0;  // the group launch: it reads half group_half(.., k) and writes the other
  for (int w = cb.carried ? 0 : 1; w < nw; w += G, ++k) {
    const int cnt = std::min(G, nw - w), t0 = s.plan.start(w);
    WinRed r{};
    WinGrp g{};
    r.nw = g.nw = cnt;
    for (int i = 0; i < cnt; ++i) {
      r.K[i] = g.K[i] = s.plan.size(w + i);
      r.slot[i] = slot(w + i);
      r.tk[i] = s.tk(w + i);
      g.rec[i] = rec(w + i);
    }
    r.p_out = w + cnt == nw ? a.p_out : nullptr;  // the rollout's last P
    hipLaunchKernelGGL(k_win_reduce_group, dim3(r.K[0], cnt), dim3(64 * ncap), 0, s.st, c->kp, r);  // (the larger windows first)
    LAUNCH_CHECK("k_win_reduce_group");
    ahead(g, w + cnt);
    if (int rc = launch_step_group(c, a.mode, false, a.act_row(t0), a.act_stride, s.tk(w), g,
                                   1 - group_half(cb.carried, cb.half, k), a.rew_row(t0), a.rew_stride, none, s.st,
                                   wts ? wts + t0 : nullptr))
      return rc;
  }
  return MDR_OK;
}

enum FirstCounts {  // where the first window's per-tick counts of a direct sequence come from
  kCountNow,        // counted here; the count kernel's last block does the P-only reduce
  kBegun,           // the same launch, already issued by mdr_rollout_begin
  kBegunAllreduced, // ... on a sharded context: P from the allreduced class totals (WinDrv::red)
  kCarried          // the whole first group, by the previous call's last step launch (CallBoundary::carried)
};

// the grouped direct sequence: an unsharded context under individual_L2 (MDR_OPT_WINDOW_GROUP)
static bool direct_grouped(const mdr_ctx* c) {
  return c->win_group > 0 && !has_comm(c) && c->world <= 1 && !win_common(c);
}

// ... whose calls may count the next call's first group (never a buffer source: the next call's action
// rows are unknown)
static bool carry_ok(const mdr_ctx* c, int mode) {
  return c->carry && direct_grouped(c) && window_ok(c, mode) && (mode == MDR_ACT_RANDOM || mode == MDR_ACT_ALWAYS_ON);
}

// the windows a carried count holds are the first group this call's plan steps (they were planned from
// the same n, window and group, so a mismatch means the record is not of this plan: count afresh)
static bool carry_plan_matches(const CarriedCount& k, const WinPlan& plan, int G) {
  if (k.nw != std::min(G, plan.count())) return false;
  for (int i = 0; i < k.nw; ++i)
    if (k.K[i] != plan.size(i)) return false;
  return true;
}

// the first window's drivers as the KA step kernels take them
static WinDrv first_window_drivers(const mdr_tick* host_ticks, int K) {
  WinDrv dv{};
  for (int j = 0; j < K; ++j) {
    const mdr_tick& h = host_ticks[j];
    dv.od_k[j] = h.t_od_prev + 273.0;  // (k_win_reduce's rec[0]: the same IEEE addition)
    dv.solar[j] = h.solar;
    dv.s_prev[j] = h.s_prev;
    if (fast_tick_ok(h.t_od_prev, h.solar)) dv.ok |= 1u << j;  // (win_tick_record's rec[3])
  }
  dv.tick0 = host_ticks[0].tick;
  return dv;
}

// The direct sequence (ids consecutive, checked by the caller): the first window's count and P-only
// reduce need only the tick ids; its step kernel then takes the drivers as kernel arguments
// (k_step_window<..., KA>), and the later windows' drivers are staged into d_ticks behind it (their
// first reader is the first step kernel's lookahead... which reads tick ids only: tick0 + K + j).
static int window_launches_direct(mdr_ctx* c, const RolloutArgs& a, const mdr_tick* host_ticks, FirstCounts first,
                                  hipStream_t st, const CallBoundary& cb = CallBoundary{}) {
  if (int rc = win_common_unsharded(c, first == kBegunAllreduced)) return rc;
  const WinSeq s{c, a, st, WinPlan(a.n, c->win)};
  const int K = s.plan.size(0), nw = s.plan.count();
  if ((first == kCarried) != cb.carried || ((cb.carried || cb.speculate) && !direct_grouped(c)))
    return fail(MDR_ESTATE, "window launches: a carried count outside the grouped direct sequence");
  SlotsGuard slots(c->v);  // dirty until the sequence is fully issued
  if (first == kCarried) {  // (no count, no KA launch: the group sequence from window 0)
    if (int rc = window_groups(s, c->win_group, WinDrv{}, host_ticks, nullptr, cb)) return rc;
    return slots.done();
  }
  if (first == kCountNow)
    if (int rc = launch_count(c, a.mode, a.action, a.act_stride, nullptr, host_ticks[0].tick, K, s.slot(0), c->d_onb,
                              c->d_wah, nullptr, st, true))
      return rc;
  WinDrv dv = first_window_drivers(host_ticks, K);
  if (nw == 1) dv.p_out = a.p_out;
  if (first == kBegunAllreduced) dv.red = win_red_ptr(c, s.slot(0));
  // an unsharded context under individual_L2: the windows in groups (MDR_OPT_WINDOW_GROUP)
  if (first != kBegunAllreduced && direct_grouped(c)) {
    if (int rc = window_groups(s, c->win_group, dv, host_ticks, nullptr, cb)) return rc;
    return slots.done();
  }
  if (int rc = s.step(0, nw > 1 ? s.plan.size(1) : 0, c->d_onb, c->d_wah, s.slot(1), &dv)) return rc;
  if (int rc = s.finish(0)) return rc;
  if (a.n > K)
    if (int rc = stage_recs(host_ticks + K, a.n - K, c->d_ticks + K, st)) return rc;
  if (int rc = s.staged_windows(1, false)) return rc;
  return slots.done();
}

// The count-ahead pipeline (sharded, comm stream present, drivers staged).  An open-loop source's FSM
// needs no thermal state, so window w's count (from the end words of window w-1) and its allreduce
// run on the comm stream, up to two windows ahead of the compute stream's tick records + step (no
// lookahead): the allreduce hides behind the step kernels.  Two buffer sets alternate; events order them.
static int window_pipeline(mdr_ctx* c, const RolloutArgs& a, hipStream_t st) {
  if (int rc = win_common_unsharded(c, true)) return rc;
  const WinSeq s{c, a, st, WinPlan(a.n, c->win)};
  const int nw = s.plan.count();
  hipStream_t cs = c->comm_stream;
  uint64_t* onbs[2] = {c->d_onb, c->d_onb2};
  uint32_t* wahs[2] = {c->d_wah, c->d_wah2};
  SlotsGuard slots(c->v);  // dirty until the sequence is fully issued
  HIP_TRY(hipEventRecord(c->ev_pc, st));  // the state and staged ticks, before the first count
  HIP_TRY(hipStreamWaitEvent(cs, c->ev_pc, 0));
  for (int w = 0; w < nw; ++w) {
    const int K = s.plan.size(w);
    // comm stream: count(w) + allreduce; count(w) reuses the buffers step(w - 2) read
    if (w >= 2) HIP_TRY(hipStreamWaitEvent(cs, c->ev_k1[(w - 2) % kSlabs], 0));
    // (the count kernel's last block sums its shards: one allreduce of K x n_cap totals, <= 1 KiB)
    if (int rc = launch_count(c, a.mode, a.act_row(s.plan.start(w)), a.act_stride, s.tk(w), 0, K, s.slot(w),
                              onbs[w % 2], wahs[w % 2], w == 0 ? nullptr : wahs[(w - 1) % 2], cs, true))
      return rc;
    if (int rc = comm_allreduce(c, win_red_ptr(c, s.slot(w)), (size_t)K * c->kp.n_cap, 0, cs)) return rc;
    HIP_TRY(hipEventRecord(c->ev_ar[w % kSlabs], cs));
    // compute stream: the tick records + step (no lookahead)
    HIP_TRY(hipStreamWaitEvent(st, c->ev_ar[w % kSlabs], 0));
    hipLaunchKernelGGL(k_win_records, dim3(1), dim3(kWindowMax), 0, st, c->kp, s.slot(w), K, s.tk(w), s.p_out(w));
    LAUNCH_CHECK("k_win_records");
    if (int rc = s.step(w, 0, onbs[w % 2], wahs[w % 2], s.slot(w))) return rc;
    HIP_TRY(hipEventRecord(c->ev_k1[w % kSlabs], st));
  }
  return slots.done();
}

// the second ON-mask / end-word set of the count-ahead pipeline (allocated on first use)
static bool pipe_buffers(mdr_ctx* c) {
  if (c->d_onb2 && c->d_wah2) return true;
  if (!c->d_onb2.reserve(c->onb_rows) &&!c->d_wah2.reserve(c->d_wah.capacity())) return true;
  (void)hipGetLastError();  // (the caller runs the windows unpipelined: no error is left behind)
  c->d_onb2.reset(), c->d_wah2.reset();  // both or neither
  return false;
}

// n ticks of a bang-bang source as ceil(n / win) closed-loop windows of near-equal size
// (WinPlan), the drivers staged in d_ticks.  Per window: k_step_closed (state in registers
// for the K ticks, raw pen_i to the reward rows, the ticks' ON counts into the count slot),
// k_win_reduce (P and the signal penalty into the tick records; it zeroes the shards it sums, so the
// one slot serves every window: stream order puts the next window's adds behind it) and
// k_closed_reward over the window's rows.  One shared row (rew_stride == 0): only the last window's
// last tick is finalised.  Kernels only, so the sequence can be captured.
// stats (mdr_rollout_stats): row t of the rollout goes to stats + t * kTickRow — the STATS
// instantiation of k_step_closed (block partials per tick into d_wstat, checked against the launch
// geometry first) and, last of the window, k_closed_stats over its K ticks.
// A common penalty mode (never with stats): the COMMON instantiation of k_step_closed (a {sum pen_i /
// N, max pen_i} pair per tick and block into d_wpen, checked against the launch geometry first),
// k_win_reduce, k_win_pen_reduce over the window's ticks (ntile = the grid: k_pen_reduce's order) and
// k_closed_reward_common over its rows — 4 nw launches; one shared row: the last window's last tick
// alone is reduced and finalised, 2 nw + 2.
static int closed_launches(mdr_ctx* c, const RolloutArgs& a, hipStream_t st, double* stats = nullptr) {
  const bool common = win_common(c);
  if (common && stats) return fail(MDR_ESTATE, "window launch: no stats rows from a common-penalty window");
  if (common && (!c->d_wpen || !c->d_wres)) return fail(MDR_ESTATE, "window launch: no penalty partial rows");
  if (stats && !c->d_wstat) return fail(MDR_ESTATE, "window launch: no stats partial rows");
  double* const wstat = stats ? c->d_wstat : nullptr;
  const WinPlan plan(a.n, c->win);
  const int nw = plan.count(), mode = a.mode;
  const int64_t rew_stride = a.rew_stride;
  const KParams kp = c->kp;
  const int ncap = kp.n_cap;
  const TickArgs* const tk = c->d_ticks;
  unsigned long long* slot = c->d_wslab;
  const double* rec = reinterpret_cast<const double*>(win_red_ptr(c, slot) + (size_t)kWindowMax * ncap);
  const unsigned grid = win_grid(c);
  SlotsGuard slots(c->v);  // dirty until the sequence is fully issued
  for (int w = 0; w < nw; ++w) {
    const int K = plan.size(w), t0 = plan.start(w);
    double* r = a.rew_row(t0);
    hipEvent_t e0, e1;
    if (int rc = step_event_pair(c, &e0, &e1)) return rc;
    // (extra: nothing, or the STATS instantiations' partial rows)
    auto closed = [&](auto kernel, auto... extra) {
      if (e0)
        hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, e0, e1, 0, kp, tk + t0, K, r, rew_stride, slot,
                              extra...);
      else
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, kp, tk + t0, K, r, rew_stride, slot, extra...);
    };
    if (stats) {  // (the partial rows this launch's geometry writes)
      if (int rc = mdr_window_stats_check(kp.n, dev_bytes(c->d_wstat))) return rc;
      if (mode == MDR_ACT_BANGBANG) closed(k_step_closed<kActBangBang, kWinHpt, true, false, double*>, wstat);
      else closed(k_step_closed<kActDeadband, kWinHpt, true, false, double*>, wstat);
    } else if (common) {  // (grid x K pairs, a quarter of what the per-wave rows of k_step_window need)
      if (int rc = mdr_window_pen_check(kp.n, dev_bytes(c->d_wpen))) return rc;
      if (mode == MDR_ACT_BANGBANG) closed(k_step_closed<kActBangBang, kWinHpt, false, true, double*>, c->d_wpen.get());
      else closed(k_step_closed<kActDeadband, kWinHpt, false, true, double*>, c->d_wpen.get());
    } else if (mode == MDR_ACT_BANGBANG) {
      closed(k_step_closed<kActBangBang, kWinHpt, false, false>);
    } else {
      closed(k_step_closed<kActDeadband, kWinHpt, false, false>);
    }
    LAUNCH_CHECK("k_step_closed");
    hipLaunchKernelGGL(k_win_reduce, dim3(K), dim3(64 * ncap), 0, st, kp, slot, K, tk + t0,
                       w == nw - 1 ? a.p_out : nullptr);
    LAUNCH_CHECK("k_win_reduce");
    if (common) {
      if (rew_stride || w == nw - 1) {
        const int j0 = rew_stride ? 0 : K - 1;
        hipLaunchKernelGGL(k_win_pen_reduce, dim3(K - j0), dim3(256), 0, st,
                           (const double*)c->d_wpen + (size_t)j0 * grid * 2, (int)grid, c->d_wres + 2 * j0);
        LAUNCH_CHECK("k_win_pen_reduce");
        hipLaunchKernelGGL(k_closed_reward_common, dim3(blocks(kp.n, 256), K - j0), dim3(256), 0, st, kp,
                           (const double*)c->d_wres, rec, j0, r, rew_stride);
        LAUNCH_CHECK("k_closed_reward_common");
      }
    } else if (rew_stride || w == nw - 1) {
      const int j0 = rew_stride ? 0 : K - 1;
      hipLaunchKernelGGL(k_closed_reward, dim3(blocks(kp.n, 256), K - j0), dim3(256), 0, st, kp, rec, j0, r,
                         rew_stride);
      LAUNCH_CHECK("k_closed_reward");
    }
    if (stats) {
      hipLaunchKernelGGL(k_closed_stats, dim3(K), dim3(kTickBlock), 0, st, kp, (const double*)wstat, (int)grid, slot,
                         stats + (size_t)t0 * kTickRow);
      LAUNCH_CHECK("k_closed_stats");
    }
  }
  return slots.done();
}

// ---- the sharded closed-loop window sequencers: a bang-bang source under
// individual_L2 on a context with a communicator, the drivers staged in d_ticks.  The window's state
// trajectory never reads the cluster power, so each rank runs k_step_closed on its own houses; only
// the reward's signal term needs the cluster's ON counts.  Window w of the WinPlan uses count slot
// w % 3: step (raw pen_i to the rows, this rank's ON counts into the slot's shards) -> sum
// (k_win_shard_sum: shards -> red, shards zeroed) -> allreduce of red's K x n_cap totals (<= 1 KiB)
// -> finish (k_closed_reward_sharded: P and the signal term from the totals, rows rewritten in
// place; the last window's last P to p_out).  One shared row (rew_stride == 0): only the last window
// is allreduced and finished (its last tick); the earlier ones sum and zero.
struct ClosedShardSeq {
  mdr_ctx* c;
  const RolloutArgs& a;
  WinPlan plan;
  double* xpart = nullptr;  // mdr_rollout_sharded_stats: this rank's partial rows X[rank][0..n) (null: no rows)
  unsigned long long* slot(int w) const { return c->d_wslab + (size_t)(w % 3) * c->wslab_len; }
  bool finished(int w) const { return a.rew_stride || w == plan.count() - 1; }
  int step(int w, hipStream_t st) const {
    const int K = plan.size(w), t0 = plan.start(w);
    const unsigned grid = win_grid(c);
    if (xpart) {  // the STATS instantiations (untouched kernels), their block partials into d_wstat
      if (int rc = mdr_window_stats_check(c->kp.n, dev_bytes(c->d_wstat))) return rc;
      if (a.mode == MDR_ACT_BANGBANG)
        hipLaunchKernelGGL((k_step_closed<kActBangBang, kWinHpt, true, false, double*>), dim3(grid), dim3(256), 0, st,
                           c->kp, (const TickArgs*)(c->d_ticks + t0), K, a.rew_row(t0), a.rew_stride, slot(w),
                           c->d_wstat.get());
      else
        hipLaunchKernelGGL((k_step_closed<kActDeadband, kWinHpt, true, false, double*>), dim3(grid), dim3(256), 0, st,
                           c->kp, (const TickArgs*)(c->d_ticks + t0), K, a.rew_row(t0), a.rew_stride, slot(w),
                           c->d_wstat.get());
    } else if (a.mode == MDR_ACT_BANGBANG)
      hipLaunchKernelGGL((k_step_closed<kActBangBang, kWinHpt, false, false>), dim3(grid), dim3(256), 0, st, c->kp,
                         (const TickArgs*)(c->d_ticks + t0), K, a.rew_row(t0), a.rew_stride, slot(w));
    else
      hipLaunchKernelGGL((k_step_closed<kActDeadband, kWinHpt, false, false>), dim3(grid), dim3(256), 0, st, c->kp,
                         (const TickArgs*)(c->d_ticks + t0), K, a.rew_row(t0), a.rew_stride, slot(w));
    LAUNCH_CHECK("k_step_closed");
    return MDR_OK;
  }
  int sum(int w, hipStream_t st) const {
    hipLaunchKernelGGL(k_win_shard_sum, dim3(plan.size(w)), dim3(64 * c->kp.n_cap), 0, st, c->kp, slot(w));
    LAUNCH_CHECK("k_win_shard_sum");
    return MDR_OK;
  }
  // the window's partial stats rows, behind sum(w) on its stream and BEFORE allreduce(w) rewrites red
  // in place with the cluster's totals (a no-op without rows)
  int part(int w, hipStream_t st) const {
    if (!xpart) return MDR_OK;
    hipLaunchKernelGGL(k_closed_stats_part, dim3(plan.size(w)), dim3(kTickBlock), 0, st, c->kp,
                       (const double*)c->d_wstat.get(), (int)win_grid(c),
                       (const unsigned long long*)win_red_ptr(c, slot(w)), xpart + (size_t)plan.start(w) * kTickRow);
    LAUNCH_CHECK("k_closed_stats_part");
    return MDR_OK;
  }
  // the window's allreduce and reward finish, both ordered on st
  int reduce_finish(int w, hipStream_t st) const {
    const int K = plan.size(w), t0 = plan.start(w), j0 = a.rew_stride ? 0 : K - 1;
    unsigned long long* red = win_red_ptr(c, slot(w));
    if (int rc = comm_allreduce(c, red, (size_t)K * c->kp.n_cap, 0, st)) return rc;
    hipLaunchKernelGGL(k_closed_reward_sharded, dim3(blocks(c->kp.n, 256), K - j0), dim3(256), 0, st, c->kp,
                       (const unsigned long long*)red, (const TickArgs*)(c->d_ticks + t0), j0, K, a.rew_row(t0),
                       a.rew_stride, w == plan.count() - 1 ? a.p_out : nullptr);
    LAUNCH_CHECK("k_closed_reward_sharded");
    return MDR_OK;
  }
};

// one stream: step -> sum -> allreduce -> finish per window
static int closed_sharded_serial(mdr_ctx* c, const RolloutArgs& a, hipStream_t st, double* xpart = nullptr) {
  const ClosedShardSeq s{c, a, WinPlan(a.n, c->win), xpart};
  SlotsGuard slots(c->v);  // dirty until the sequence is fully issued
  for (int w = 0; w < s.plan.count(); ++w) {
    if (int rc = s.step(w, st)) return rc;
    if (int rc = s.sum(w, st)) return rc;
    if (int rc = s.part(w, st)) return rc;
    if (s.finished(w))
      if (int rc = s.reduce_finish(w, st)) return rc;
  }
  return slots.done();
}

// two streams, a reward row per tick (rew_stride != 0: every window is finished): the compute stream
// runs step(w) -> sum(w), the comm stream allreduce(w) -> finish(w) behind sum(w)'s event.
// step(w + 1) and sum(w + 1) are issued BEFORE the host enters allreduce(w): a host-callback
// communicator synchronises the comm stream and blocks in the collective, and the device then has
// the next window to run.  Hazards: sum(w + 3) rewrites the red part of slot w % 3, which
// allreduce(w) and finish(w) use — it waits for finish(w)'s event (the shards step(w + 3) adds to
// were zeroed by sum(w), earlier on the compute stream); finish(w) and step(w + 1) write disjoint
// rows.  The caller's stream is the compute stream and waits for the last finish.
// (One shared row has a single allreduce and finish, behind the last step: nothing to run beside
// them, and the two stream hand-offs measured 8 % of a 1M-house call — mdr_rollout_sharded sends it
// to closed_sharded_serial.)
// With stats rows, part(w) sits on the compute stream behind sum(w) and before ev_k1[w]: it has read
// red before allreduce(w) starts, and d_wstat before step(w + 1) rewrites it.
static int closed_sharded_pipeline(mdr_ctx* c, const RolloutArgs& a, hipStream_t st, double* xpart = nullptr) {
  const ClosedShardSeq s{c, a, WinPlan(a.n, c->win), xpart};
  const int nw = s.plan.count();
  hipStream_t cs = c->comm_stream;
  SlotsGuard slots(c->v);  // dirty until the sequence is fully issued
  auto compute = [&](int w) -> int {
    if (int rc = s.step(w, st)) return rc;
    if (w >= 3) HIP_TRY(hipStreamWaitEvent(st, c->ev_ar[(w - 3) % kSlabs], 0));
    if (int rc = s.sum(w, st)) return rc;
    if (int rc = s.part(w, st)) return rc;
    HIP_TRY(hipEventRecord(c->ev_k1[w % kSlabs], st));
    return MDR_OK;
  };
  if (int rc = compute(0)) return rc;
  for (int w = 0; w < nw; ++w) {
    if (w + 1 < nw)
      if (int rc = compute(w + 1)) return rc;
    HIP_TRY(hipStreamWaitEvent(cs, c->ev_k1[w % kSlabs], 0));
    if (int rc = s.reduce_finish(w, cs)) return rc;
    HIP_TRY(hipEventRecord(c->ev_ar[w % kSlabs], cs));
  }
  HIP_TRY(hipStreamWaitEvent(st, c->ev_ar[(nw - 1) % kSlabs], 0));
  return slots.done();
}

// (per-tick stats rows, defined with mdr_tick_stats below)
static int check_tick_stats_ctx(mdr_ctx* c, const char* who);
static int tick_scratch(mdr_ctx* c);
static int launch_tick_stats(mdr_ctx* c, const double* reward, const double* p_dev, double p_host, double* row,
                             hipStream_t st);
static int launch_tick_partials(mdr_ctx* c, const double* reward, double* partial, unsigned* nb_out, hipStream_t st);
static int rows_scratch(mdr_ctx* c);
// (stats rows on a sharded context, defined with mdr_tick_stats_sharded below)
static int check_stats_rows(const char* who, int64_t n, int64_t stats_rows, int64_t stats_row0);
static int stats_exchange_reserve(mdr_ctx* c, int m, const char* who);
static double* stats_part_rows(mdr_ctx* c, int m, int row);
static int stats_rows_exchange(mdr_ctx* c, int m, bool closed, double* rows, hipStream_t st);

// The launch sequence of a rollout with staged drivers (d_ticks), so a captured graph is reusable:
// the window sequence (open-loop sources), the closed-loop window sequence (bang-bang sources under
// individual_L2), or one step launch per tick (+ phase 1 where no lookahead counts ahead).
// stats (mdr_rollout_stats; never on the open-loop window sequence): row t -> stats + t * kTickRow,
// by the closed-loop windows themselves, or per tick by mdr_tick_stats' two kernels behind the
// tick's step (and its finalise kernels in the common penalty modes), every tick's P on the device.
// ret (mdr_rollout_returns' one launch per tick, whatever the window sequences could do): a.reward is
// one context-owned row; behind each tick's final reward k_return_acc adds weights[t] times the row to
// `returns`.
struct ReturnsAcc {
  const double* weights;  // host, a.n
  double* returns;
};
static int rollout_launches(mdr_ctx* c, const RolloutArgs& a, hipStream_t st, double* stats = nullptr,
                            const ReturnsAcc* ret = nullptr) {
  const int n = a.n, mode = a.mode;
  if (!ret && window_ok(c, mode)) return window_launches(c, a, false, st);
  if (!ret && closed_ok(c, mode, stats != nullptr)) return closed_launches(c, a, st, stats);
  double* const p_tick = a.p_out ? a.p_out : c->d_stat_p;  // (stats: every tick's P, for its row)
  if (int rc = zero_slabs(c, st)) return rc;
  c->v.slabs_zeroed();
  const bool la = lookahead_ok(mode);
  for (int t = 0; t < n; ++t) {
    const uint8_t* act = a.act_row(t);
    double* r = a.rew_row(t);
    if (!la || t == 0)
      if (int rc = launch_counts(c, act, mode, 0, c->d_ticks + t, st)) return rc;
    hipEvent_t e0, e1;  // (around the tick's group of launches, recorded on the stream)
    if (int rc = step_event_pair(c, &e0, &e1)) return rc;
    if (e0) HIP_TRY(hipEventRecord(e0, st));
    int rc = launch_step(c, act, mode, TickArgs{}, c->d_ticks + t, r, la ? mode : 0, MDR_CTRL_NONE,
                         nullptr, stats ? p_tick : t == n - 1 ? a.p_out : nullptr, st);
    if (rc) return rc;
    if (win_common(c)) {  // step_tensor's common-penalty tail, the tick's drivers read from d_ticks
      hipLaunchKernelGGL(k_pen_reduce, dim3(1), dim3(256), 0, st, c->d_pen_partial, c->pen_blocks, c->d_partial2);
      LAUNCH_CHECK("k_pen_reduce");
      hipLaunchKernelGGL(k_reward_finalize_dev, dim3(blocks(c->kp.n, 256)), dim3(256), 0, st, c->kp,
                         (const TickArgs*)(c->d_ticks + t), (const unsigned long long*)slab_at(c, c->v.ring() - 1),
                         (const double*)c->d_partial2, r);
      LAUNCH_CHECK("k_reward_finalize");
    }
    if (stats)  // the post-step state, this tick's reward row and P: mdr_tick_stats' launches
      if (int rc2 = launch_tick_stats(c, r, p_tick, 0.0, stats + (size_t)t * kTickRow, st)) return rc2;
    if (ret) {
      hipLaunchKernelGGL(k_return_acc, dim3(blocks(c->kp.n, 256)), dim3(256), 0, st, (int64_t)c->kp.n, ret->weights[t],
                         (const double*)r, ret->returns);
      LAUNCH_CHECK("k_return_acc");
    }
    if (e1) HIP_TRY(hipEventRecord(e1, st));
  }
  return MDR_OK;
}

static bool consecutive(const mdr_tick* ticks, int n) {
  for (int i = 1; i < n; ++i)
    if (ticks[i].tick != ticks[0].tick + (uint64_t)i) return false;
  return true;
}

// the buffers a rollout with stats rows needs, allocated outside any capture: the closed-loop
// windows' block partials, or the per-tick form's k_tick_stats partials and a P scalar
static int rollout_stats_scratch(mdr_ctx* c, int mode, bool need_p) {
  if (closed_ok(c, mode, true)) {
    return dev_reserve(c->d_wstat, mdr_window_stats_bytes(c->kp.n) / sizeof(double), "d_wstat");
  }
  if (need_p)
    if (int rc = dev_reserve(c->d_stat_p, 1, "d_stat_p")) return rc;
  return tick_scratch(c);
}

// who writes the stats rows of a rollout from this action source, or why nobody does
static int rollout_stats_path(mdr_ctx* c, int mode, const std::string& who) {
  if (int rc = check_tick_stats_ctx(c, who.c_str())) return rc;
  if (window_ok(c, mode))
    return fail(MDR_EARG, who + ": no stats rows from the open-loop window rollout (k_step_window); use the "
                                "bang-bang sources, or mdr_set_rollout_window(0) for one launch per tick");
  return closed_ok(c, mode, true) ? MDR_STATS_CLOSED_WINDOWS : MDR_STATS_PER_TICK;
}

int mdr_rollout_stats_path(mdr_ctx* c, int mode) {
  if (!c) return fail(MDR_EARG, "mdr_rollout_stats_path: null ctx");
  if (int rc_ = cluster_ready(c, "mdr_rollout_stats_path")) return rc_;
  if (!check_mode(mode)) return fail(MDR_EARG, "mdr_rollout_stats_path: bad action source");
  return rollout_stats_path(c, mode, "mdr_rollout_stats");
}

// a common penalty mode on a sharded context: its mean / max penalty would be shard-local
static bool common_sharded(const mdr_ctx* c) { return win_common(c) && (has_comm(c) || c->world > 1); }

// The argument checks the rollout entry points share, in the order a call with several faults
// reports them.  ptrs: the entry point's own pointer arguments are there.
enum {
  kDropBegun = 1,    // discard an early count once the arguments are there (the others settle it themselves)
  kShardedOnly = 2,  // mdr_rollout_sharded: a communicator
  kNoCommon = 4,     // no common penalty mode (mdr_rollout / mdr_rollout_begin decide behind the preamble)
  kSettlesCarry = 8  // mdr_rollout / mdr_rollout_begin: the caller consumes or drops a carried count itself
};
static int rollout_preamble(mdr_ctx* c, const char* who, bool ptrs, const RolloutArgs& a, int flags) {
  if (!c || !ptrs || a.n < 1) return fail(MDR_EARG, std::string(who) + ": bad argument");
  if (flags & kDropBegun) c->v.drop_early_count();
  c->v.state_may_change((flags & kSettlesCarry) != 0);
  if (int rc_ = cluster_ready(c, std::string(who))) return rc_;
  if ((flags & kShardedOnly) && !has_comm(c))
    return fail(MDR_ESTATE, std::string(who) + ": no communicator (mdr_rccl_init / mdr_comm_host)");
  if (!check_mode(a.mode) || (a.mode == MDR_ACT_BUFFER && !a.action))
    return fail(MDR_EARG, std::string(who) + ": bad action source");
  if ((flags & kNoCommon) && win_common(c)) return fail(MDR_EARG, std::string(who) + ": common penalty modes need the per-step API");
  return MDR_OK;
}

// The first window counted ahead by mdr_rollout_begin for exactly this call?  (Its count took the
// ids tick0 + j and its P-only reduce consumed the slot's shards: only the direct sequence can follow
// it, whatever use_graph asks.)  sharded: a single window, its counts allreduced already.
static bool begun_matches(const mdr_ctx* c, const RolloutArgs& a, const mdr_tick* ticks, bool sharded) {
  const EarlyCount& b = c->v.early();
  return b.on && b.sharded == sharded && b.n == a.n && b.mode == a.mode && b.tick0 == ticks[0].tick &&
         b.action == a.action && b.act_stride == a.act_stride && (!sharded || (has_comm(c) && a.n <= c->win)) &&
         window_ok(c, a.mode) && consecutive(ticks, a.n);
}

// (stats == nullptr: mdr_rollout, its launches and graph keys)
int mdr_rollout_stats(mdr_ctx* c, int n, const mdr_tick* ticks, const uint8_t* action, int64_t act_stride,
                      int mode, double* reward, int64_t rew_stride, double* p_out, double* stats, int row0,
                      int use_graph, void* stream) {
  const RolloutArgs a{n, action, act_stride, mode, reward, rew_stride, p_out};
  const char* const who = stats ? "mdr_rollout_stats" : "mdr_rollout";
  if (int rc = rollout_preamble(c, who, ticks && a.reward, a, kSettlesCarry)) return rc;
  hipStream_t st = S(stream);
  // the direct sequence, and the first group counted by the previous call for exactly this one?
  const bool direct_seq = !stats && !use_graph && window_ok(c, a.mode) && consecutive(ticks, a.n);
  const bool may_carry = direct_seq && carry_ok(c, a.mode);
  const bool carried = may_carry && c->v.carry_matches(a.n, a.mode, ticks[0].tick, c->win, c->win_group, st) &&
                       carry_plan_matches(c->v.carry(), WinPlan(a.n, c->win), c->win_group);
  CallBoundary cb{};
  if (carried) {
    cb.carried = true;
    cb.slot_base = c->v.carry().slot_base;
    cb.half = c->v.carry().half;
    c->v.carry_consumed();
  } else {
    c->v.drop_carry();  // an unmatched one: its shards are cleared below
  }
  // speculate only behind a call this one continues: one-off and irregular callers never pay for it
  cb.speculate = may_carry && c->v.continues_direct(a.n, a.mode, ticks[0].tick, c->win, c->win_group, st);
  c->v.direct_call_forgotten();
  if (stats) {
    if (row0 < 0) return fail(MDR_EARG, std::string(who) + ": row0 < 0");
    if (int rc = rollout_stats_path(c, a.mode, who); rc < 0) return rc;
  }
  if (common_sharded(c))
    return fail(MDR_EARG, std::string(who) + ": common penalty modes on a sharded context need the per-step API");
  double* const srow = stats ? stats + (size_t)row0 * kTickRow : nullptr;
  const bool counted = !carried && begun_matches(c, a, ticks, false);
  if (counted) c->v.early_consumed();
  else c->v.drop_early_count();  // an unmatched early count: its shards are cleared below
  Sequence seq(c->v, Sequence::kRollout);
  int rc = refresh_if_dirty(c, st);
  if (rc) return rc;
  if (counted || direct_seq) {
    rc = ensure_ticks(c, a.n);
    if (!rc) rc = wslab_clean(c, st);
    if (!rc) rc = window_launches_direct(c, a, ticks, carried ? kCarried : counted ? kBegun : kCountNow, st, cb);
    if (!rc && may_carry) {  // the shape the next call must continue, and what this one counted for it
      const WinPlan plan(a.n, c->win);
      const uint64_t next = ticks[0].tick + (uint64_t)a.n;
      c->v.direct_call_issued(DirectCall{true, a.n, a.mode, c->win, c->win_group, next, st});
      if (cb.speculate) {
        CarriedCount k{true, a.n, a.mode, next, c->win, c->win_group, std::min(c->win_group, plan.count()), {},
                       carry_slot(cb.slot_base, plan.count()), st,
                       group_half(cb.carried, cb.half, group_launches(cb.carried, plan.count(), c->win_group))};
        for (int i = 0; i < k.nw; ++i) k.K[i] = plan.size(i);
        c->v.carry_counted(k);
      }
    }
    return seq.end(rc);
  }
  rc = stage_ticks(c, a.n, ticks, st);
  if (!rc) rc = wslab_clean(c, st);
  if (!rc && stats) rc = rollout_stats_scratch(c, a.mode, !a.p_out);
  if (rc) return rc;
  if (!use_graph) return seq.end(rollout_launches(c, a, st, srow));
  return seq.end(replay_graph(c, c->graphs, 0, GraphKey{a, stats, stats ? row0 : 0},
                              [&](hipStream_t cs) { return rollout_launches(c, a, cs, srow); }, st));
}

int mdr_rollout(mdr_ctx* c, int n, const mdr_tick* ticks, const uint8_t* action, int64_t act_stride,
                int mode, double* reward, int64_t rew_stride, double* p_out, int use_graph, void* stream) {
  return mdr_rollout_stats(c, n, ticks, action, act_stride, mode, reward, rew_stride, p_out, nullptr, 0, use_graph, stream);
}

// ---- rollouts that accumulate per-house discounted returns
// which sequence a returns call from this action source takes (the ticks' ids consecutive)
static int returns_path(const mdr_ctx* c, int mode) {
  if (!win_common(c) && window_ok(c, mode)) return MDR_RETURNS_GROUPED;
  if (!win_common(c) && closed_ok(c, mode)) return MDR_RETURNS_CLOSED_WINDOWS;
  return MDR_RETURNS_PER_TICK;
}

int mdr_rollout_returns_path(mdr_ctx* c, int mode) {
  if (!c) return fail(MDR_EARG, "mdr_rollout_returns_path: null ctx");
  if (int rc_ = cluster_ready(c, "mdr_rollout_returns_path")) return rc_;
  if (!check_mode(mode)) return fail(MDR_EARG, "mdr_rollout_returns_path: bad action source");
  return returns_path(c, mode);
}

// the weight row (whole staging records) and the scratch row, grown outside any launch sequence;
// queued work may still read the old buffers, so a growth synchronises first (no graph holds them)
static int returns_scratch(mdr_ctx* c, int n_ticks, bool row) {
  const size_t need_w = ((size_t)n_ticks + 3) / 4 * 4, need_r = row ? (size_t)c->kp.n : 0;
  if (need_w <= c->d_ret_w.capacity() && need_r <= c->d_ret_row.capacity()) return MDR_OK;
  HIP_TRY(hipDeviceSynchronize());
  if (int rc = dev_reserve(c->d_ret_w, need_w < 128 ? 128 : need_w, "d_ret_w")) return rc;
  return need_r ? dev_reserve(c->d_ret_row, need_r, "d_ret_row") : MDR_OK;
}

// The grouped direct sequence with k_step_group_ret: window_launches_direct's grouped branch, the
// weights staged by value ahead of everything (they depend on the call's arguments alone), groups of
// one window under MDR_OPT_WINDOW_GROUP 0.  a.reward: the returns row (a.rew_stride 0).
static int returns_group_launches(mdr_ctx* c, const RolloutArgs& a, const mdr_tick* host_ticks, const double* weights,
                                  hipStream_t st) {
  const WinSeq s{c, a, st, WinPlan(a.n, c->win)};
  const int K = s.plan.size(0), nw = s.plan.count();
  std::vector<double> wpad(((size_t)a.n + 3) / 4 * 4, 0.0);
  std::copy(weights, weights + a.n, wpad.begin());
  SlotsGuard slots(c->v);  // dirty until the sequence is fully issued
  if (int rc = stage_recs(wpad.data(), (int)(wpad.size() / 4), c->d_ret_w, st)) return rc;
  if (int rc = launch_count(c, a.mode, a.action, a.act_stride, nullptr, host_ticks[0].tick, K, s.slot(0), c->d_onb,
                            c->d_wah, nullptr, st, true))
    return rc;
  WinDrv dv = first_window_drivers(host_ticks, K);
  if (nw == 1) dv.p_out = a.p_out;
  if (int rc = window_groups(s, c->win_group > 0 ? c->win_group : 1, dv, host_ticks, c->d_ret_w)) return rc;
  return slots.done();
}

// The closed-loop windows of a returns call (closed_launches' rules: a bang-bang source under
// individual_L2, drivers and weights staged): per window k_step_closed<..., ClosedRet> (a_i to the scratch row),
// k_win_reduce, k_closed_return.  The one count slot serves every window, as there.
static int returns_closed_launches(mdr_ctx* c, const RolloutArgs& a, hipStream_t st) {
  const WinPlan plan(a.n, c->win);
  const int nw = plan.count(), ncap = c->kp.n_cap;
  const KParams kp = c->kp;
  const TickArgs* const tk = c->d_ticks;
  const double* const wts = c->d_ret_w;
  unsigned long long* slot = c->d_wslab;
  const double* rec = reinterpret_cast<const double*>(win_red_ptr(c, slot) + (size_t)kWindowMax * ncap);
  const unsigned grid = win_grid(c);
  SlotsGuard slots(c->v);  // dirty until the sequence is fully issued
  for (int w = 0; w < nw; ++w) {
    const int K = plan.size(w), t0 = plan.start(w);
    const ClosedRet cr{wts + t0};
    if (a.mode == MDR_ACT_BANGBANG)
      hipLaunchKernelGGL((k_step_closed<kActBangBang, kWinHpt, false, false, ClosedRet>), dim3(grid), dim3(256), 0, st, kp,
                         tk + t0, K, (double*)c->d_ret_row, (int64_t)0, slot, cr);
    else
      hipLaunchKernelGGL((k_step_closed<kActDeadband, kWinHpt, false, false, ClosedRet>), dim3(grid), dim3(256), 0, st, kp,
                         tk + t0, K, (double*)c->d_ret_row, (int64_t)0, slot, cr);
    LAUNCH_CHECK("k_step_closed<ClosedRet>");
    hipLaunchKernelGGL(k_win_reduce, dim3(K), dim3(64 * ncap), 0, st, kp, slot, K, tk + t0,
                       w == nw - 1 ? a.p_out : nullptr);
    LAUNCH_CHECK("k_win_reduce");
    hipLaunchKernelGGL(k_closed_return, dim3(blocks(kp.n, 256)), dim3(256), 0, st, kp, rec, wts + t0, K,
                       (const double*)c->d_ret_row, a.reward);
    LAUNCH_CHECK("k_closed_return");
  }
  return slots.done();
}

int mdr_rollout_returns(mdr_ctx* c, int n, const mdr_tick* ticks, const uint8_t* action, int64_t act_stride, int mode,
                        const double* weights, double* returns, double* p_out, void* stream) {
  const char* const who = "mdr_rollout_returns";
  RolloutArgs a{n, action, act_stride, mode, returns, 0, p_out};
  // what needs no context first, so each refusal names its argument (all before any HIP call)
  if (n < 1) return fail(MDR_EARG, std::string(who) + ": n_ticks < 1");
  if (!weights || !returns) return fail(MDR_EARG, std::string(who) + ": null weights or returns");
  if (!check_mode(mode)) return fail(MDR_EARG, std::string(who) + ": unknown action source");
  if (mode == MDR_ACT_BUFFER && !action) return fail(MDR_EARG, std::string(who) + ": a buffer source without actions");
  if (int rc = rollout_preamble(c, who, ticks != nullptr, a, 0)) return rc;
  if (has_comm(c) || c->world > 1)
    return fail(MDR_ESTATE, std::string(who) + ": a sharded context (communicator attached) has no returns rollout");
  hipStream_t st = S(stream);
  c->v.drop_early_count();  // (an early count is mdr_rollout's: its shards are cleared below)
  int path = returns_path(c, a.mode);
  if (path == MDR_RETURNS_GROUPED && !consecutive(ticks, a.n)) path = MDR_RETURNS_PER_TICK;  // (the KA count takes ids)
  if (int rc = returns_scratch(c, a.n, path != MDR_RETURNS_GROUPED)) return rc;
  Sequence seq(c->v, Sequence::kRollout);
  int rc = refresh_if_dirty(c, st);
  if (rc) return rc;
  if (path == MDR_RETURNS_GROUPED) {
    rc = ensure_ticks(c, a.n);
    if (!rc) rc = wslab_clean(c, st);
    if (!rc) rc = returns_group_launches(c, a, ticks, weights, st);
    return seq.end(rc);
  }
  rc = stage_ticks(c, a.n, ticks, st);
  if (!rc) rc = wslab_clean(c, st);
  if (rc) return rc;
  if (path == MDR_RETURNS_CLOSED_WINDOWS) {
    std::vector<double> wpad(((size_t)a.n + 3) / 4 * 4, 0.0);
    std::copy(weights, weights + a.n, wpad.begin());
    rc = stage_recs(wpad.data(), (int)(wpad.size() / 4), c->d_ret_w, st);
    if (!rc) rc = returns_closed_launches(c, a, st);
    return seq.end(rc);
  }
  const ReturnsAcc ret{weights, returns};
  a.reward = c->d_ret_row;  // the tick's rewards, one row every tick overwrites
  return seq.end(rollout_launches(c, a, st, nullptr, &ret));
}

// The first window's FSM counts (and its cluster power P) of an mdr_rollout of n ticks from tick
// id tick0, launched before the host has the ticks' drivers (they only need the tick ids), so the
// count overlaps the host work.  The next mdr_rollout with the same (n, mode, action, tick0) skips
// them; any other call discards them.  A no-op (returns 0) when the rollout will not take the
// temporally blocked path.
int mdr_rollout_begin(mdr_ctx* c, int n, uint64_t tick0, const uint8_t* action, int64_t act_stride, int mode,
                      void* stream) {
  const RolloutArgs a{n, action, act_stride, mode, nullptr, 0, nullptr};
  if (int rc = rollout_preamble(c, "mdr_rollout_begin", true, a, kSettlesCarry)) return rc;
  c->v.drop_early_count();  // a previous one that no rollout consumed
  // the previous call counted this call's first group already: nothing to launch (mdr_rollout checks the
  // rest — the tick ids, no graph — and drops the carry if it is not the call announced here)
  // (action / act_stride are not compared: carry_ok admits random and always_on only, which read no action rows)
  if (carry_ok(c, mode) && c->v.carry_matches(n, mode, tick0, c->win, c->win_group, S(stream))) return MDR_OK;
  c->v.drop_carry();  // its shards are cleared below, or before the next rollout
  if (!window_ok(c, mode)) return MDR_OK;
  // a sharded context (RCCL attached): single-window rollouts only, counts allreduced here, so
  // the matching mdr_rollout_sharded launches just the KA step kernel
  const bool sharded = has_comm(c);
  if (sharded && n > c->win) return MDR_OK;
  if (common_sharded(c)) return MDR_OK;  // (mdr_rollout / _sharded refuse these)
  hipStream_t st = S(stream);
  Sequence seq(c->v);
  int rc = refresh_if_dirty(c, st);
  if (!rc) rc = wslab_clean(c, st);
  if (rc) return rc;
  const int k0 = WinPlan(n, c->win).size(0);
  SlotsGuard slots(c->v);
  // the window's P (the counts need no drivers): the matching direct mdr_rollout then launches the
  // step kernel with the drivers as arguments (k_step_window<..., KA>), nothing in between — on one
  // GPU the count kernel's last block reduces; sharded, the reduce follows the counts' allreduce
  rc = launch_count(c, mode, action, act_stride, nullptr, tick0, k0, c->d_wslab, c->d_onb, c->d_wah, nullptr, st,
                    true);
  if (rc) return rc;
  if (sharded) {  // every rank's per-tick class totals (its count kernel's last block), summed
    // (the KA step derives each tick's P from these totals itself: no k_win_records launch, r06)
    if (int rc2 = comm_allreduce(c, win_red_ptr(c, c->d_wslab), (size_t)k0 * c->kp.n_cap, 0, st)) return rc2;
  }
  slots.done();
  c->v.early_counted(EarlyCount{true, n, mode, tick0, action, act_stride, sharded});
  return seq.ok();
}

// Measurement: one rollout as direct launches (no graph, drivers staged first) with an event pair
// around every step-kernel launch (k_step_window on the window path, k_step_* per tick otherwise);
// *ms = the summed kernel time, *launches = the number of step launches.  Synchronises on the last
// event.
int mdr_time_step_kernels(mdr_ctx* c, int n, const mdr_tick* ticks, const uint8_t* action, int64_t act_stride,
                          int mode, double* reward, int64_t rew_stride, void* stream, float* ms, int* launches) {
  enter_writer(c);  // (a refused call discards an early count too)
  const RolloutArgs a{n, action, act_stride, mode, reward, rew_stride, nullptr};
  if (int rc = rollout_preamble(c, "mdr_time_step_kernels", ticks && reward && ms && launches, a, 0)) return rc;
  if (common_sharded(c))  // (mdr_rollout's refusal)
    return fail(MDR_EARG, "mdr_time_step_kernels: common penalty modes on a sharded context need the per-step API");
  hipStream_t st = S(stream);
  Sequence seq(c->v, Sequence::kRollout);
  int rc = refresh_if_dirty(c, st);
  if (!rc) rc = stage_ticks(c, n, ticks, st);
  if (!rc) rc = wslab_clean(c, st);
  if (rc) return rc;
  std::vector<hipEvent_t> evs;
  c->step_events = &evs;
  rc = rollout_launches(c, a, st);
  c->step_events = nullptr;
  float total = 0.0f;
  if (!rc && !evs.empty() && hipEventSynchronize(evs.back()) != hipSuccess) rc = fail(MDR_EHIP, "event sync");
  for (size_t i = 0; !rc && i + 1 < evs.size(); i += 2) {
    float e = 0.0f;
    if (hipEventElapsedTime(&e, evs[i], evs[i + 1]) != hipSuccess) rc = fail(MDR_EHIP, "event elapsed");
    total += e;
  }
  for (hipEvent_t e : evs) hipEventDestroy(e);
  if (rc) return rc;
  *ms = total;
  *launches = (int)(evs.size() / 2);
  return seq.ok();
}

// ------------------------------------------------------------------------------------ obs
static ObsArgs obs_args(const mdr_ctx* c, const mdr_obs_spec* sp, const mdr_obs_scalars* sc) {
  ObsArgs o{};
  o.n_feat = sp->n_feat;
  o.msg_w = mdr_msg_width(sp);
  o.n_comm = sp->n_comm;
  o.comm_mode = sp->comm_mode;
  o.hvac_state = sp->hvac_state;
  o.solar_state = sp->solar_state;
  o.thermal_state = sp->thermal_state;
  o.msg_thermal = sp->msg_thermal;
  o.msg_hvac = sp->msg_hvac;
  o.comm_table = sp->comm_table;
  o.halo_msg = sp->halo_msg;
  o.halo_next = nullptr;
  o.msg_all = sp->msg_all;
  o.norm_reg_sig = sp->norm_reg_sig;
  o.cfg_ua = sp->cfg_ua;
  o.cfg_ca = sp->cfg_ca;
  o.cfg_cm = sp->cfg_cm;
  o.cfg_hm = sp->cfg_hm;
  o.cfg_cop = c->cfg.cop;
  o.cfg_lcf = c->cfg.lcf;
  o.cfg_cap = sp->cfg_cap;
  if (sc) { o.p = sc->p; o.s = sc->s; o.solar = sc->solar; o.t_od = sc->t_od; }
  return o;
}

int mdr_msg_width(const mdr_obs_spec* sp) {
  if (!sp) return 0;
  return 4 + (sp->msg_thermal ? 4 : 0) + (sp->msg_hvac ? 3 : 0);
}

static int expected_feat(const mdr_obs_spec* sp) {
  int base = 10 + (sp->hvac_state ? 2 : 0) + (sp->solar_state ? 1 : 0) + (sp->thermal_state ? 5 : 0);
  return base + sp->n_comm * mdr_msg_width(sp);
}

static int check_obs_spec(const mdr_obs_spec* sp, const char* who) {
  if (sp->n_feat != expected_feat(sp)) return fail(MDR_EARG, std::string(who) + ": n_feat does not match the flags");
  if (sp->n_comm < 0 || sp->n_comm > 64) return fail(MDR_EARG, std::string(who) + ": n_comm out of range");
  if (sp->comm_mode == MDR_COMM_TABLE && sp->n_comm > 0 && !sp->comm_table)
    return fail(MDR_EARG, std::string(who) + ": TABLE mode without a table");
  if (sp->comm_mode == MDR_COMM_TABLE && mdr_msg_width(sp) > 16) return fail(MDR_EARG, std::string(who) + ": msg width");
  return MDR_OK;
}

int mdr_obs(mdr_ctx* c, const mdr_obs_spec* sp, const mdr_obs_scalars* sc, const double* p_dev,
            float* obs, void* stream) {
  if (!c || !sp || !sc || !obs) return fail(MDR_EARG, "mdr_obs: null argument");
  if (int rc_ = cluster_ready(c, "mdr_obs")) return rc_;
  if (int rc = check_obs_spec(sp, "mdr_obs")) return rc;
  ObsArgs o = obs_args(c, sp, sc);
  const int lo = sp->n_comm / 2, hi = (sp->n_comm + 1) / 2;
  size_t tile = ((size_t)kObsBlock * sp->n_feat + 3) & ~(size_t)3;
  size_t msg = (size_t)(lo + kObsBlock + hi) * o.msg_w;
  size_t bytes = (tile + msg) * sizeof(float);
  if (bytes > 160 * 1024) return fail(MDR_EARG, "mdr_obs: obs row too wide for one LDS tile");
  hipLaunchKernelGGL(k_obs, dim3(blocks(c->kp.n, kObsBlock)), dim3(kObsBlock), bytes, S(stream), c->kp, o,
                     p_dev, obs);
  LAUNCH_CHECK("k_obs");
  return MDR_OK;
}

int mdr_msg_pack(mdr_ctx* c, const mdr_obs_spec* sp, float* out, void* stream) {
  if (!c || !sp || !out) return fail(MDR_EARG, "mdr_msg_pack: null argument");
  if (int rc_ = cluster_ready(c, "mdr_msg_pack")) return rc_;
  ObsArgs o = obs_args(c, sp, nullptr);
  if (o.msg_w > 16) return fail(MDR_EARG, "mdr_msg_pack: message wider than 16");
  hipLaunchKernelGGL(k_msg_pack, dim3(blocks(c->kp.n, 256)), dim3(256), 0, S(stream), c->kp, o, out);
  LAUNCH_CHECK("k_msg_pack");
  return MDR_OK;
}

int mdr_halo_pack(mdr_ctx* c, const mdr_obs_spec* sp, float* out, void* stream) {
  if (!c || !sp || !out) return fail(MDR_EARG, "mdr_halo_pack: null argument");
  ObsArgs o = obs_args(c, sp, nullptr);
  const int lo = sp->n_comm / 2, hi = (sp->n_comm + 1) / 2;
  if (lo + hi == 0) return MDR_OK;
  hipLaunchKernelGGL(k_halo_pack, dim3(1), dim3(64), 0, S(stream), c->kp, o, lo, hi, out);
  LAUNCH_CHECK("k_halo_pack");
  return MDR_OK;
}

// ------------------------------------------------------------------------------------ batch
// E independent clusters of <= kBatchMaxLen houses in one context, one launch per rollout call
// (mdr.h "environment batches").
size_t mdr_batch_stride(int64_t env_len) { return env_len < 1 ? 0 : (size_t)((env_len + 127) / 128 * 128); }

static int batch_ready(const mdr_ctx* c, const char* who) {
  if (!c->bound) return fail(MDR_ESTATE, std::string(who) + ": context not bound");
  if (!c->batch.n_envs) return fail(MDR_ESTATE, std::string(who) + ": no batch declared (mdr_batch_set)");
  return MDR_OK;
}

// room for n elements in a buffer queued work may still read: synchronise, then reserve
extern "C++" template <class T>
static int batch_reserve(Dev<T>& b, size_t n, const char* name) {
  if (n <= b.capacity()) return MDR_OK;
  HIP_TRY(hipDeviceSynchronize());
  return dev_reserve(b, n, name);
}

int mdr_batch_set(mdr_ctx* c, int32_t n_envs, int32_t env_len, const uint64_t* seeds) {
  enter_writer(c);
  if (!c || !seeds) return fail(MDR_EARG, "mdr_batch_set: null argument");
  if (!c->bound) return fail(MDR_ESTATE, "mdr_batch_set: context not bound");
  if (n_envs < 1) return fail(MDR_EARG, "mdr_batch_set: n_envs < 1");
  if (env_len < 1 || env_len > kBatchMaxLen)
    return fail(MDR_EARG, "mdr_batch_set: env_len outside 1..1024 (a cluster is stepped by one workgroup)");
  static_assert(kBatchMaxLen == MDR_BATCH_MAX_LEN, "the header's limit is the kernels'");
  const int64_t stride = (int64_t)mdr_batch_stride(env_len);
  if (c->kp.n != (int64_t)n_envs * stride || c->kp.n_global != c->kp.n || c->kp.goff != 0)
    return fail(MDR_EARG, "mdr_batch_set: the context must have n_local = n_global = n_envs * mdr_batch_stride(env_len), offset 0");
  if (win_common(c)) return fail(MDR_EARG, "mdr_batch_set: the common penalty modes are not batched (individual_L2 only)");
  if (has_comm(c) || c->world > 1) return fail(MDR_EARG, "mdr_batch_set: a context with a communicator holds no batch");
  const KParams& k = c->kp;
  const uintptr_t al = (uintptr_t)k.t_air | (uintptr_t)k.t_mass | (uintptr_t)k.hvac | (uintptr_t)k.ua | (uintptr_t)k.ca |
                       (uintptr_t)k.cm | (uintptr_t)k.hm | (uintptr_t)k.target | (uintptr_t)k.cap_idx;
  if (al & 15) return fail(MDR_EARG, "mdr_batch_set: the bound arrays must be 16-byte aligned");
  HIP_TRY(hipSetDevice(c->cfg.device));
  if (int rc = batch_reserve(c->d_batch_seeds, (size_t)n_envs, "d_batch_seeds")) return rc;
  HIP_TRY(hipDeviceSynchronize());  // (a queued launch may still read the old keys)
  HIP_TRY(hipMemcpy(c->d_batch_seeds, seeds, (size_t)n_envs * sizeof(uint64_t), hipMemcpyHostToDevice));
  destroy_graphs(c);
  c->batch = BatchArgs{n_envs, env_len, (int)stride, c->d_batch_seeds};
  c->v.state_replaced();  // (nothing the single-cluster sequences derived is of this layout)
  return MDR_OK;
}

// refresh_if_dirty over the clusters' houses (the pads hold nothing)
static int batch_refresh_if_dirty(mdr_ctx* c, hipStream_t st) {
  if (!c->v.coef_dirty()) return MDR_OK;
  HIP_TRY(hipMemsetAsync(c->d_flags, 0, sizeof(int), st));
  hipLaunchKernelGGL(k_batch_refresh, dim3(blocks(c->kp.n, 256)), dim3(256), 0, st, c->kp, c->batch, c->d_flags);
  LAUNCH_CHECK("k_batch_refresh");
  c->v.coef_refreshed();
  return MDR_OK;
}
static_assert(sizeof(TickArgs) == sizeof(mdr_tick), "mdr_tick records are copied as TickArgs");

// k_batch_rollout<A> for a run-time source
static void launch_batch_rollout(int mode, dim3 grid, dim3 block, hipStream_t st, const KParams& kp, const BatchArgs& b,
                                 const TickArgs* tk, int n, const uint8_t* action, int64_t act_stride, double* reward,
                                 int64_t rew_stride, double* p_out) {
#define MDR_LAUNCH_BATCH(A) \
  hipLaunchKernelGGL((k_batch_rollout<A>), grid, block, 0, st, kp, b, tk, n, action, act_stride, reward, rew_stride, p_out)
  switch (mode) {
    case MDR_ACT_BUFFER: MDR_LAUNCH_BATCH(MDR_ACT_BUFFER); break;
    case MDR_ACT_RANDOM: MDR_LAUNCH_BATCH(MDR_ACT_RANDOM); break;
    case MDR_ACT_ALWAYS_ON: MDR_LAUNCH_BATCH(MDR_ACT_ALWAYS_ON); break;
    case MDR_ACT_BANGBANG: MDR_LAUNCH_BATCH(kActBangBang); break;
    default: MDR_LAUNCH_BATCH(kActDeadband); break;
  }
#undef MDR_LAUNCH_BATCH
}

int mdr_batch_rollout(mdr_ctx* c, int n, const mdr_tick* ticks, const uint8_t* action, int64_t act_stride, int mode,
                      double* reward, int64_t rew_stride, double* p_out, void* stream) {
  enter_writer(c);
  if (!c || !ticks || !reward || !p_out || n < 1) return fail(MDR_EARG, "mdr_batch_rollout: bad argument");
  if (int rc = batch_ready(c, "mdr_batch_rollout")) return rc;
  if (!check_mode(mode) || (mode == MDR_ACT_BUFFER && !action))
    return fail(MDR_EARG, "mdr_batch_rollout: bad action source");
  if (((uintptr_t)reward & 15) || (rew_stride & 1))
    return fail(MDR_EARG, "mdr_batch_rollout: reward rows must be 16-byte aligned (an even rew_stride)");
  if ((int64_t)c->batch.n_envs * n > ((int64_t)1 << 27)) return fail(MDR_EARG, "mdr_batch_rollout: n_envs * n_ticks > 2^27");
  hipStream_t st = S(stream);
  const size_t nrec = (size_t)c->batch.n_envs * (size_t)n;
  if (int rc = batch_reserve(c->d_batch_ticks, nrec, "d_batch_ticks")) return rc;
  Sequence seq(c->v, Sequence::kRollout);
  if (int rc = batch_refresh_if_dirty(c, st)) return rc;
  // stream order: an earlier launch reading d_batch_ticks on st precedes this write
  HIP_TRY(hipMemcpyAsync(c->d_batch_ticks, ticks, nrec * sizeof(TickArgs), hipMemcpyHostToDevice, st));
  const dim3 grid((unsigned)c->batch.n_envs), block(64u * blocks(c->batch.env_len, 128));
  launch_batch_rollout(mode, grid, block, st, c->kp, c->batch, c->d_batch_ticks.get(), n, action, act_stride, reward,
                       rew_stride, p_out);
  LAUNCH_CHECK("k_batch_rollout");
  return seq.ok();
}

// k_batch_eval<A, F> for a run-time source and form (F = 1 .. 3)
extern "C++" template <int F>
static void launch_batch_eval(int mode, dim3 grid, dim3 block, hipStream_t st, const KParams& kp, const BatchArgs& b,
                              const TickArgs* tk, int n, const uint8_t* action, int64_t act_stride, double* reward,
                              int64_t rew_stride, double* p_out, const BatchEval& ev) {
#define MDR_LAUNCH_EVAL(A)                                                                                       \
  hipLaunchKernelGGL((k_batch_eval<A, F>), grid, block, 0, st, kp, b, tk, n, action, act_stride, reward, rew_stride, \
                     p_out, ev)
  switch (mode) {
    case MDR_ACT_BUFFER: MDR_LAUNCH_EVAL(MDR_ACT_BUFFER); break;
    case MDR_ACT_RANDOM: MDR_LAUNCH_EVAL(MDR_ACT_RANDOM); break;
    case MDR_ACT_ALWAYS_ON: MDR_LAUNCH_EVAL(MDR_ACT_ALWAYS_ON); break;
    case MDR_ACT_BANGBANG: MDR_LAUNCH_EVAL(kActBangBang); break;
    default: MDR_LAUNCH_EVAL(kActDeadband); break;
  }
#undef MDR_LAUNCH_EVAL
}

int mdr_batch_rollout_eval(mdr_ctx* c, int n, const mdr_tick* ticks, const uint8_t* action, int64_t act_stride, int mode,
                           double* reward, int64_t rew_stride, const double* weights, double* returns, double* stats,
                           int stats_cap, int stats_row0, double* p_out, void* stream) {
  const char* const who = "mdr_batch_rollout_eval";
  enter_writer(c);
  // what needs no context first, so each refusal names its argument (all before any HIP call)
  if (!c || !ticks || !p_out) return fail(MDR_EARG, std::string(who) + ": null ctx, ticks or p_out");
  if (n < 1) return fail(MDR_EARG, std::string(who) + ": n_ticks < 1");
  if (!check_mode(mode)) return fail(MDR_EARG, std::string(who) + ": unknown action source");
  if (mode == MDR_ACT_BUFFER && !action) return fail(MDR_EARG, std::string(who) + ": a buffer source without actions");
  if (!reward && !returns && !stats)
    return fail(MDR_EARG, std::string(who) + ": no output (reward, returns and stats all null)");
  if (!weights != !returns) return fail(MDR_EARG, std::string(who) + ": weights and returns go together");
  if (reward && returns) return fail(MDR_EARG, std::string(who) + ": reward rows and returns exclude each other");
  if (stats && (stats_row0 < 0 || stats_cap < 0 || stats_row0 > stats_cap - n))
    return fail(MDR_EARG, std::string(who) + ": stats_row0 .. stats_row0 + n_ticks outside [0, stats_cap)");
  if (((uintptr_t)reward & 15) || (reward && (rew_stride & 1)))
    return fail(MDR_EARG, std::string(who) + ": reward rows must be 16-byte aligned (an even rew_stride)");
  if ((uintptr_t)returns & 15) return fail(MDR_EARG, std::string(who) + ": returns must be 16-byte aligned");
  if (int rc = batch_ready(c, who)) return rc;
  if ((int64_t)c->batch.n_envs * n > ((int64_t)1 << 27)) return fail(MDR_EARG, std::string(who) + ": n_envs * n_ticks > 2^27");
  hipStream_t st = S(stream);
  // the tick records, then (returns forms) the weights, in one context-owned buffer of 32-byte records
  const size_t nrec = (size_t)c->batch.n_envs * (size_t)n;
  const size_t wrec = returns ? (nrec + 3) / 4 : 0;
  if (int rc = batch_reserve(c->d_batch_ticks, nrec + wrec, "d_batch_ticks")) return rc;
  Sequence seq(c->v, Sequence::kRollout);
  if (int rc = batch_refresh_if_dirty(c, st)) return rc;
  // stream order: an earlier launch reading d_batch_ticks on st precedes these writes
  HIP_TRY(hipMemcpyAsync(c->d_batch_ticks, ticks, nrec * sizeof(TickArgs), hipMemcpyHostToDevice, st));
  double* const d_wts = reinterpret_cast<double*>(c->d_batch_ticks.get() + nrec);
  if (returns) HIP_TRY(hipMemcpyAsync(d_wts, weights, nrec * sizeof(double), hipMemcpyHostToDevice, st));
  const dim3 grid((unsigned)c->batch.n_envs), block(64u * blocks(c->batch.env_len, 128));
  const BatchEval ev{returns ? d_wts : nullptr, returns, stats, stats_cap, stats_row0};
  // rows alone are k_batch_rollout's; stats alone is the rows + stats form without a reward row
  const int form = (stats ? kBatchStats : 0) | (returns ? kBatchRet : 0);
  const TickArgs* const tk = c->d_batch_ticks.get();
  if (form == 0)
    launch_batch_rollout(mode, grid, block, st, c->kp, c->batch, tk, n, action, act_stride, reward, rew_stride, p_out);
  else if (form == kBatchStats)
    launch_batch_eval<kBatchStats>(mode, grid, block, st, c->kp, c->batch, tk, n, action, act_stride, reward, rew_stride,
                                   p_out, ev);
  else if (form == kBatchRet)
    launch_batch_eval<kBatchRet>(mode, grid, block, st, c->kp, c->batch, tk, n, action, act_stride, nullptr, 0, p_out, ev);
  else
    launch_batch_eval<kBatchStats | kBatchRet>(mode, grid, block, st, c->kp, c->batch, tk, n, action, act_stride, nullptr, 0,
                                               p_out, ev);
  LAUNCH_CHECK(form ? "k_batch_eval" : "k_batch_rollout");
  return seq.ok();
}

int mdr_batch_obs(mdr_ctx* c, const mdr_obs_spec* sp, const mdr_obs_scalars* sc, const double* p_dev, float* obs,
                  void* stream) {
  if (!c || !sp || !sc || !obs) return fail(MDR_EARG, "mdr_batch_obs: null argument");
  if (int rc = batch_ready(c, "mdr_batch_obs")) return rc;
  if (int rc = check_obs_spec(sp, "mdr_batch_obs")) return rc;
  if (sp->comm_mode != MDR_COMM_RING || sp->halo_msg || sp->msg_all)
    return fail(MDR_EARG, "mdr_batch_obs: the ring (neighbours) topology inside each cluster only");
  ObsArgs o = obs_args(c, sp, nullptr);
  const int lo = sp->n_comm / 2, hi = (sp->n_comm + 1) / 2;
  const size_t tile = ((size_t)kObsBlock * sp->n_feat + 3) & ~(size_t)3;
  const size_t msg = (size_t)(lo + kObsBlock + hi) * o.msg_w;
  const size_t bytes = (tile + msg) * sizeof(float);
  if (bytes > 160 * 1024) return fail(MDR_EARG, "mdr_batch_obs: obs row too wide for one LDS tile");
  if (c->batch.n_envs > 65535) return fail(MDR_EARG, "mdr_batch_obs: more than 65,535 clusters (the grid's second dimension)");
  hipStream_t st = S(stream);
  static_assert(sizeof(mdr_obs_scalars) == 4 * sizeof(double), "the scalars are staged as rows of 4 doubles");
  if (int rc = batch_reserve(c->d_batch_sc, (size_t)c->batch.n_envs * 4, "d_batch_sc")) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_batch_sc, sc, (size_t)c->batch.n_envs * sizeof(mdr_obs_scalars), hipMemcpyHostToDevice,
                         st));
  hipLaunchKernelGGL(k_batch_obs, dim3(blocks(c->batch.env_len, kObsBlock), (unsigned)c->batch.n_envs), dim3(kObsBlock),
                     bytes, st, c->kp, o, c->batch, c->d_batch_sc.get(), p_dev, obs);
  LAUNCH_CHECK("k_batch_obs");
  return MDR_OK;
}

// ------------------------------------------------------------------------------------ greedy
}  // extern "C"

namespace {

// The greedy order: a stable sort of (key, house) pairs (hipCUB / rocprim radix sort; at 2^20
// houses rocprim runs its block merge sort, which measured faster here than forcing Onesweep:
// 212 us vs ~250 us incl. its per-pass lookback resets, profiles/r02g_greedy_kernel_stats.csv)
hipError_t greedy_sort(void* tmp, size_t& bytes, const double* kin, double* kout, const int* vin, int* vout,
                       int64_t n, hipStream_t st) {
  return hipcub::DeviceRadixSort::SortPairs(tmp, bytes, kin, kout, vin, vout, (int)n, 0, 64, st);
}

// the greedy scratch is one unit: emptied as a whole, with its capacities
void greedy_clear(mdr_ctx* c) {
  c->g_key.reset(), c->g_key2.reset(), c->g_ps.reset(), c->g_incl.reset();
  c->g_idx.reset(), c->g_idx2.reset(), c->g_ls.reset(), c->g_tmp.reset();
  c->g_kpos.reset(), c->g_extra.reset();
  c->g_part.reset(), c->g_hist.reset(), c->g_sel_rec.reset(), c->g_win.reset();
  c->g_sorted.reset(), c->g_map.reset(), c->g_range.reset(), c->g_tickets.reset();
  c->g_sel = nullptr;
  c->g_cap = 0, c->gq_parts_cap = 0;
}

int greedy_scratch(mdr_ctx* c, int64_t n) {
  if (c->g_cap >= n) return MDR_OK;
  c->v.scratch_regrown();
  const int rc = grow_unit([&] { greedy_clear(c); }, [&]() -> int {
    if (int rc = dev_reserve(c->g_key, n, "g_key")) return rc;
    if (int rc = dev_reserve(c->g_key2, n, "g_key2")) return rc;
    if (int rc = dev_reserve(c->g_ps, n, "g_ps")) return rc;
    if (int rc = dev_reserve(c->g_incl, n, "g_incl")) return rc;
    if (int rc = dev_reserve(c->g_idx, n, "g_idx")) return rc;
    if (int rc = dev_reserve(c->g_idx2, n, "g_idx2")) return rc;
    if (int rc = dev_reserve(c->g_ls, n, "g_ls")) return rc;
    if (int rc = dev_reserve(c->g_kpos, 2, "g_kpos")) return rc;
    if (int rc = dev_reserve(c->g_extra, 64, "g_extra")) return rc;
    // (min, max) partials: k_gq_keys' grid, or the grid of the step kernel whose epilogue writes the
    // keys (k_step_pipe: a block per kStepGqWaves x tpw x 128 houses, tpw >= 2)
    const int parts = (int)std::max<int64_t>(kGqParts, (n + 1023) / 1024);
    if (int rc = dev_reserve(c->g_part, 2 * (size_t)parts, "g_part")) return rc;
    c->gq_parts_cap = parts;
    if (int rc = dev_reserve(c->g_hist, kGqHistWords, "g_hist", true)) return rc;  // (the kernels re-zero what they read)
    if (int rc = dev_reserve(c->g_sel_rec, kGqSelBytes, "g_sel")) return rc;
    c->g_sel = reinterpret_cast<GqSel*>(c->g_sel_rec.get());
    if (int rc = dev_reserve(c->g_map, kGqCells, "g_map")) return rc;
    unsigned char init[kGqSelBytes] = {};
    uint32_t map[kGqCells];
    gq_sel_init(init, map);
    HIP_TRY(hipMemcpy(c->g_sel, init, kGqSelBytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->g_map, map, sizeof(map), hipMemcpyHostToDevice));
    if (int rc = dev_reserve(c->g_win, kGqCap + 1, "g_win")) return rc;  // (sharded: [0] = the count header)
    if (int rc = dev_reserve(c->g_range, 2, "g_range")) return rc;
    if (int rc = dev_reserve(c->g_tickets, kTicketWords, "g_tickets", true)) return rc;
    if (int rc = dev_reserve(c->g_sorted, kGqCap, "g_sorted")) return rc;
    size_t b1 = 0, b2 = 0;
    HIP_TRY(greedy_sort(nullptr, b1, c->g_key, c->g_key2, c->g_idx, c->g_idx2, n, nullptr));
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, b2, c->g_ps.get(), c->g_incl.get(), (int)n));
    return dev_reserve(c->g_tmp, b1 > b2 ? b1 : b2, "g_tmp");
  });
  if (!rc) c->g_cap = n;
  return rc;
}

// before a producer (k_gq_keys, the step's GQ epilogue) adds to g_hist: counts an earlier producer
// left unconsumed (two GQ steps with no greedy call between, or keys dropped by a state change)
// are zeroed first, so the select never sees the sum of two states
int gq_hist_produce(mdr_ctx* c, hipStream_t st) {
  if (c->v.hist_add()) {
    hipLaunchKernelGGL(k_zero_u64, dim3(64), dim3(256), 0, st, reinterpret_cast<unsigned long long*>(c->g_hist.get()),
                       (int64_t)(kGqHistWords / 2));
    LAUNCH_CHECK("k_zero_u64 (g_hist)");
  }
  return MDR_OK;
}

// the keys and superbin histogram of the current state (when no step epilogue prepared them);
// slab: zeroed for the decisions' counts (nullptr: none)
int launch_gq_keys(mdr_ctx* c, hipStream_t st, unsigned long long* slab, bool local_map) {
  if (int rc = gq_hist_produce(c, st)) return rc;
  hipLaunchKernelGGL(k_gq_keys, dim3(kGqParts), dim3(kGqThreads), 0, st, c->kp, gq_codes(c), c->g_part, c->g_hist,
                     c->g_sel, c->g_map, slab);
  LAUNCH_CHECK("k_gq_keys");
  // (sharded, local_map = false: every rank's map must stay the one built from the allreduced range)
  if (c->v.map_stale() && local_map) {  // (a written state: cells over its key range, then the codes again)
    unsigned char* sel = reinterpret_cast<unsigned char*>(c->g_sel);
    hipLaunchKernelGGL(k_gq_remap, dim3(1), dim3(256), 0, st, c->kp, (const double*)c->g_part, (int)kGqParts,
                       c->g_hist + kGqBins * 4, c->g_sel, c->g_map,
                       reinterpret_cast<double*>(sel + gq_kmin_offset(-1)), reinterpret_cast<double*>(sel + gq_scale_offset(-1)));
    LAUNCH_CHECK("k_gq_remap");
    hipLaunchKernelGGL(k_gq_keys, dim3(kGqParts), dim3(kGqThreads), 0, st, c->kp, gq_codes(c), c->g_part, c->g_hist,
                       c->g_sel, c->g_map, slab);
    LAUNCH_CHECK("k_gq_keys (remapped)");
    c->v.maps_fitted();
  }
  c->v.keys_from_kernel(kGqParts, slab != nullptr);
  return MDR_OK;
}

}  // namespace

extern "C" {

int mdr_ctrl_greedy(mdr_ctx* c, double budget, uint8_t* action, void* stream) {
  if (!c || !action) return fail(MDR_EARG, "mdr_ctrl_greedy: null argument");
  if (int rc_ = cluster_ready(c, "mdr_ctrl_greedy")) return rc_;
  const bool keys_ready = c->v.take_keys() && c->g_cap >= c->kp.n;  // (the last step's epilogue wrote them)
  enter_writer(c);
  Sequence seq(c->v);
  int rc = greedy_scratch(c, c->kp.n);
  if (rc) return rc;
  hipStream_t st = S(stream);
  const int n = (int)c->kp.n;
  double pmin = INFINITY;
  for (int k = 0; k < c->cfg.n_cap; ++k) pmin = fmin(pmin, c->cfg.cap_table[k] / c->cfg.cop);
  unsigned long long* slab = slab_at(c, c->v.ring());  // the counts of the actions decided here
  if (c->kp.n_cap <= 4 && !c->greedy_sort) {
    // histogram select (mdr_kernels.hip k_gq_*): no sort of the whole cluster, no host
    // synchronisation; k_gq_select decides exactly what the candidate window cannot
    if (!keys_ready) {
      if (int rc2 = launch_gq_keys(c, st, slab)) return rc2;
    } else if (!c->v.slab_zeroed()) {
      // the producing step counted a lookahead into this slab: the decisions replace those counts
      hipLaunchKernelGGL(k_zero_u64, dim3(1), dim3(256), 0, st, slab, (int64_t)c->slab_len);
      LAUNCH_CHECK("k_zero_u64 (decision slab)");
    }
    // the slab was zeroed by the codes' producer (k_gq_keys, or the GQ step: its next slab is this)
    const int nstage = (n + kGqStage - 1) / kGqStage;
    if (c->gq_band && !c->gq_band_skip) {
      // the band's two launches: binsc (window from the band and compaction, or the bins), finish
      // (rank + decide, or on a miss window + compaction + decide)
      hipLaunchKernelGGL(k_gq_binsc, dim3(nstage), dim3(kGqThreads), 0, st, c->kp, gq_codes(c), c->g_hist, budget,
                         c->g_sel, c->g_win, action, slab);
      LAUNCH_CHECK("k_gq_binsc");
      hipLaunchKernelGGL(k_gq_finish, dim3(kGqSelBlocks), dim3(1024), 0, st, c->kp, (const uint32_t*)gq_codes(c),
                         c->g_win, c->g_sorted, budget, pmin, c->g_sel, action, slab, c->g_hist, c->g_tickets,
                         (const double*)c->g_part, c->v.nparts(), c->g_map);
      LAUNCH_CHECK("k_gq_finish");
      c->v.hist_consumed();
      c->v.counts_produced();
      return seq.ok();
    } else {
      hipLaunchKernelGGL(k_gq_bins, dim3(kGqParts), dim3(kGqThreads), 0, st, c->kp, gq_codes(c), c->g_hist, budget,
                         c->g_sel, slab);
      LAUNCH_CHECK("k_gq_bins");
    }
    hipLaunchKernelGGL(k_gq_compact, dim3(nstage), dim3(kGqThreads), 0, st, c->kp, gq_codes(c), c->g_hist, budget,
                       c->g_sel, c->g_win, action, slab);
    LAUNCH_CHECK("k_gq_compact");
    // the window ranked by 256 blocks, the last of them decides (a one-block select measured slower:
    // DESIGN.md §3.3)
    hipLaunchKernelGGL(k_gq_select, dim3(kGqSelBlocks), dim3(1024), 0, st, c->kp, (const uint4*)c->g_win,
                       c->g_sorted, budget, pmin, c->g_sel, action, slab, c->g_hist, (const uint4*)nullptr, 0,
                       c->g_tickets, (const double*)c->g_part, c->v.nparts(), c->g_map);
    LAUNCH_CHECK("k_gq_select");
    c->v.hist_consumed();
    c->v.counts_produced();
    return seq.ok();
  }
  hipLaunchKernelGGL(k_greedy_keys, dim3(blocks(n, 256)), dim3(256), 0, st, c->kp, c->g_key, c->g_idx);
  LAUNCH_CHECK("k_greedy_keys");
  size_t b = c->g_tmp.capacity();
  HIP_TRY(greedy_sort(c->g_tmp, b, c->g_key, c->g_key2, c->g_idx, c->g_idx2, n, st));
  hipLaunchKernelGGL(k_greedy_gather, dim3(blocks(n, 256)), dim3(256), 0, st, c->kp, c->g_idx2, c->g_ps,
                     c->g_ls);
  LAUNCH_CHECK("k_greedy_gather");
  b = c->g_tmp.capacity();
  HIP_TRY(hipcub::DeviceScan::InclusiveSum(c->g_tmp.get(), b, c->g_ps.get(), c->g_incl.get(), n, st));
  hipLaunchKernelGGL(k_greedy_walk, dim3(1), dim3(256), 0, st, (int64_t)n, c->g_incl, c->g_ps, c->g_ls,
                     budget, pmin, c->g_kpos, c->g_extra, 64);
  LAUNCH_CHECK("k_greedy_walk");
  hipLaunchKernelGGL(k_greedy_apply, dim3(blocks(n, 256)), dim3(256), 0, st, (int64_t)n, c->g_idx2,
                     c->g_kpos, c->g_extra, action);
  LAUNCH_CHECK("k_greedy_apply");
  // the counts of these actions, as the histogram form leaves them
  HIP_TRY(hipMemsetAsync(slab, 0, c->slab_len * sizeof(unsigned long long), st));
  if (int rc2 = launch_counts(c, action, MDR_ACT_BUFFER, 0, nullptr, st)) return rc2;
  c->v.counts_produced();
  return seq.ok();
}

int mdr_greedy_diag(mdr_ctx* c, uint64_t* out) {
  if (!c || !out) return fail(MDR_EARG, "mdr_greedy_diag: null argument");
  for (int k = 0; k < 4; ++k) out[k] = 0;
  if (!c->g_sel) return MDR_OK;
  unsigned char h[kGqSelBytes];
  HIP_TRY(hipMemcpy(h, c->g_sel, kGqSelBytes, hipMemcpyDeviceToHost));
  gq_diag_of(h, out);
  return MDR_OK;
}

int mdr_greedy_state(mdr_ctx* c, uint64_t* out) {
  if (!c || !out) return fail(MDR_EARG, "mdr_greedy_state: null argument");
  for (int k = 0; k < 12; ++k) out[k] = 0;
  if (!c->g_sel) return MDR_OK;
  unsigned char h[kGqSelBytes];
  HIP_TRY(hipMemcpy(h, c->g_sel, kGqSelBytes, hipMemcpyDeviceToHost));
  gq_state_of(h, out);
  return MDR_OK;
}

// config C3's loop in one call: per tick, GreedyMyopic on the current state with the tick's
// pre-step signal as budget (greedy_myopic_controller.py:67-104; the signal the obs carries), then
// the step with those actions (environment.py:86-106), whose epilogue writes the next call's keys
// — Environment.greedy_actions + step_tensor(ctrl='greedy_keys') per tick, without a host round
// trip between them
}  // extern "C"

namespace {
// the fused tick's buffers (mdr_kernels.h GqfBufs), for a cluster of n houses: one unit, but for the
// stamps (mdr_greedy_fused_stamps), which outlive a regrow
void gqf_clear(mdr_ctx* c) {
  c->fz_regions.reset(), c->fz_bkt.reset(), c->fz_mbkt.reset(), c->fz_maps.reset(), c->fz_sel.reset(), c->fz_dec.reset();
  c->fz = GqfBufs{};
  c->fz.stamps = c->fz_stamps;
  c->fz_cap_n = 0;
}

int gqf_scratch(mdr_ctx* c, int64_t n) {
  if (c->fz_cap_n >= n) return MDR_OK;
  HIP_TRY(hipDeviceSynchronize());
  c->v.fused_scratch_regrown();
  // bucket capacity: 4x the houses a (copy, bin) holds on average under an equi-depth map, >= 32
  const int64_t avg = (n + (int64_t)gq_bins_eff(c->kp.n_global) * kGqCopies - 1) / ((int64_t)gq_bins_eff(c->kp.n_global) * kGqCopies);
  const int cap = (int)std::max<int64_t>(32, 4 * avg);
  const size_t nb = (size_t)kGqCopies * kGqBand * 64 * cap;
  const int rc = grow_unit([&] { gqf_clear(c); }, [&]() -> int {
    if (int rc = dev_reserve(c->fz_regions, 2 * (size_t)kGqfParWords + kGqfMissWords, "fz.par", true)) return rc;
    if (int rc = dev_reserve(c->fz_bkt, 2 * nb, "fz.bkt")) return rc;
    if (int rc = dev_reserve(c->fz_mbkt, (size_t)kGqCopies * 128 * cap, "fz.mbkt")) return rc;
    if (int rc = dev_reserve(c->fz_maps, 2 * (size_t)kGqCells, "fz.map")) return rc;
    if (int rc = dev_reserve(c->fz_sel, kGqSelBytes, "fz.sel")) return rc;
    unsigned char init[kGqSelBytes] = {};
    uint32_t map[kGqCells];
    gqf_sel_init(init, map);
    HIP_TRY(hipMemcpy(c->fz_sel, init, kGqSelBytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->fz_maps, map, sizeof(map), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->fz_maps + kGqCells, map, sizeof(map), hipMemcpyHostToDevice));
    return dev_reserve(c->fz_dec, (size_t)n, "fz.dec");
  });
  if (rc) return rc;
  unsigned* par = c->fz_regions;  // the kernels' views, once the unit is whole
  c->fz = GqfBufs{{par, par + kGqfParWords}, par + 2 * kGqfParWords, {c->fz_bkt, c->fz_bkt + nb}, c->fz_mbkt,
                  {c->fz_maps, c->fz_maps + kGqCells}, reinterpret_cast<GqSel*>(c->fz_sel.get()), c->fz_dec,
                  cap, cap, c->fz_stamps};
  c->fz_cap_n = n;
  return MDR_OK;
}

// the fused tick's step: k_step_pipe<..., GQ = 2> applying the decision of parity par, producing 1 - par
int launch_step_fused(mdr_ctx* c, const TickArgs& tk, double* reward, uint8_t* act_out, double* p_out, int par,
                      hipStream_t st) {
  const KParams kp = c->kp;
  const int tpw = c->tpw >= 4 ? 4 : 2;
  const unsigned nb = blocks(blocks(kp.n, 128), kStepGqWaves * tpw);
  if ((int)nb > c->gq_parts_cap) return fail(MDR_ESTATE, "fused greedy: the step grid exceeds the partials buffer");
  GqOut go{act_out, nullptr, c->g_part, nullptr, nullptr, nullptr};
  unsigned long long *cur = slab_at(c, c->v.ring()), *nxt = slab_at(c, c->v.ring() + 1), *zer = slab_at(c, c->v.ring() + 2);
  if (tpw >= 4)
    hipLaunchKernelGGL((k_step_pipe<4, MDR_ACT_BUFFER, 0, 2>), dim3(nb), dim3(64 * kStepGqWaves), 0, st, kp,
                       (const uint8_t*)c->fz.dec, tk, (const TickArgs*)nullptr, cur, reward, p_out, nxt, zer, go, c->fz, par);
  else
    hipLaunchKernelGGL((k_step_pipe<2, MDR_ACT_BUFFER, 0, 2>), dim3(nb), dim3(64 * kStepGqWaves), 0, st, kp,
                       (const uint8_t*)c->fz.dec, tk, (const TickArgs*)nullptr, cur, reward, p_out, nxt, zer, go, c->fz, par);
  LAUNCH_CHECK("k_step_pipe (fused greedy)");
  c->v.fused_step_issued((int)nb);
  return MDR_OK;
}
}  // namespace

extern "C" {

// diagnostics: record k_gq_decide2's per-block phase clocks (100 MHz) of the following calls into a
// device buffer of kGqSelBlocks x kGqfStampWords words (n = 0: stop); read it back with mdr_greedy_fused_stamps
int mdr_greedy_fused_stamps(mdr_ctx* c, int on, uint64_t* out) {
  if (!c) return fail(MDR_EARG, "mdr_greedy_fused_stamps: null ctx");
  if (out && c->fz.stamps)
    HIP_TRY(hipMemcpy(out, c->fz.stamps, kGqSelBlocks * kGqfStampWords * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (on)
    if (int rc = dev_reserve(c->fz_stamps, (size_t)kGqSelBlocks * kGqfStampWords, "fz.stamps", true)) return rc;
  if (!on && c->fz.stamps) {
    HIP_TRY(hipDeviceSynchronize());
    c->fz_stamps.reset();
  }
  c->fz.stamps = c->fz_stamps;
  return MDR_OK;
}

int mdr_greedy_fused_diag(mdr_ctx* c, uint64_t* out) {
  if (!c || !out) return fail(MDR_EARG, "mdr_greedy_fused_diag: null argument");
  for (int k = 0; k < 6; ++k) out[k] = 0;
  if (!c->fz.sel) return MDR_OK;
  unsigned char h[kGqSelBytes];
  HIP_TRY(hipMemcpy(h, c->fz.sel, kGqSelBytes, hipMemcpyDeviceToHost));
  gqf_diag_of(h, out);
  return MDR_OK;
}

// The rows of a greedy rollout (stats != NULL): behind tick t's step (and finalise)
// kernels, k_tick_stats into slot t mod kTickRowsBatch of the context's partial slab, that tick's P
// into the same slot of the P slab, and k_tick_rows_finish after every kTickRowsBatch ticks and
// after the last one, a block per tick.  A batch's slots are rewritten only by launches issued
// behind its finish on the same stream.
static int greedy_rows_tick(mdr_ctx* c, int t, int n, const double* r, double* stats, double* p_out, hipStream_t st) {
  const int slot = t % kTickRowsBatch;
  unsigned nb = 0;
  if (int rc = launch_tick_partials(c, r, c->d_rows_part + (size_t)slot * kTickBlocks * kStats, &nb, st)) return rc;
  if (slot == kTickRowsBatch - 1 || t == n - 1) {
    hipLaunchKernelGGL(k_tick_rows_finish, dim3(slot + 1), dim3(kTickBlock), 0, st, (const double*)c->d_rows_part,
                       (int)nb, (const double*)c->d_rows_p, stats + (size_t)(t - slot) * kTickRow,
                       t == n - 1 ? p_out : nullptr);
    LAUNCH_CHECK("k_tick_rows_finish");
  }
  return MDR_OK;
}

// mdr_greedy_rollout (stats == NULL) and mdr_greedy_rollout_stats (stats = the row of the call's
// first tick): without rows, launch for launch the sequence as it was before there were any
static int greedy_rollout_seq(mdr_ctx* c, int n, const mdr_tick* ticks, uint8_t* action, int64_t act_stride,
                              double* reward, int64_t rew_stride, double* p_out, double* stats, void* stream) {
  hipStream_t st = S(stream);
  // the fused tick (MDR_OPT_GQ_FUSED): individual_L2 on the software-pipelined step, <= 4 classes
  const bool fused = c->gq_fused && !c->greedy_sort && c->kp.n_cap <= 4 && c->tpw >= 1 && c->fastdiv &&
                     c->kp.penalty_mode == MDR_PEN_INDIVIDUAL_L2 && n > 0;
  if (fused) {
    const bool ready = c->v.take_fused() && c->fz_cap_n >= c->kp.n;  // (the last step produced this state's counts)
    enter_writer(c);
    Sequence seq(c->v, Sequence::kRollout);
    if (int rc = refresh_if_dirty(c, st)) return rc;
    if (int rc = greedy_scratch(c, c->kp.n)) return rc;  // (the partials, tickets and sorted window)
    if (int rc = gqf_scratch(c, c->kp.n)) return rc;
    double pmin = INFINITY;
    for (int k = 0; k < c->cfg.n_cap; ++k) pmin = fmin(pmin, c->cfg.cap_table[k] / c->cfg.cop);
    int par = c->v.fused_parity();
    if (!ready) {  // the current state's keys: the producer without a step, into parity par
      hipLaunchKernelGGL(k_zero_u64, dim3(64), dim3(256), 0, st, reinterpret_cast<unsigned long long*>(c->fz.par[par]),
                         (int64_t)(kGqfParWords / 2));
      LAUNCH_CHECK("k_zero_u64 (fused producer region)");
      const unsigned g = blocks(c->kp.n, kGqStage);
      hipLaunchKernelGGL(k_gq_keys2, dim3(g), dim3(kGqThreads), 0, st, c->kp, c->fz, par, c->g_part, slab_at(c, c->v.ring()));
      LAUNCH_CHECK("k_gq_keys2");
      if (c->v.map_stale()) {  // (a written state: parity par's cells over its key range, then the producer again)
        unsigned char* fs = reinterpret_cast<unsigned char*>(c->fz.sel);
        hipLaunchKernelGGL(k_gq_remap, dim3(1), dim3(256), 0, st, c->kp, (const double*)c->g_part, (int)g, c->fz.par[par],
                           c->fz.sel, c->fz.map[par], reinterpret_cast<double*>(fs + gq_kmin_offset(par)),
                           reinterpret_cast<double*>(fs + gq_scale_offset(par)));
        LAUNCH_CHECK("k_gq_remap (fused)");
        hipLaunchKernelGGL(k_zero_u64, dim3(64), dim3(256), 0, st, reinterpret_cast<unsigned long long*>(c->fz.par[par]),
                           (int64_t)(kGqfParWords / 2));
        LAUNCH_CHECK("k_zero_u64 (fused producer region, remapped)");
        hipLaunchKernelGGL(k_gq_keys2, dim3(g), dim3(kGqThreads), 0, st, c->kp, c->fz, par, c->g_part, slab_at(c, c->v.ring()));
        LAUNCH_CHECK("k_gq_keys2 (remapped)");
        c->v.maps_fitted();
      }
      c->v.fused_keys_from_kernel((int)g);
    }
    for (int t = 0; t < n; ++t) {
      hipLaunchKernelGGL(k_gq_decide2, dim3(kGqSelBlocks), dim3(1024), 0, st, c->kp, c->fz, par, ticks[t].s_prev, pmin,
                         slab_at(c, c->v.ring()), c->g_tickets, (const double*)c->g_part, c->v.nparts());
      LAUNCH_CHECK("k_gq_decide2");
      double* r = reward + (int64_t)t * rew_stride;
      if (int rc = launch_step_fused(c, to_tick(&ticks[t]), r, action ? action + (int64_t)t * act_stride : nullptr,
                                     stats ? c->d_rows_p + t % kTickRowsBatch : p_out, par, st))
        return rc;
      par = 1 - par;
      if (stats)
        if (int rc = greedy_rows_tick(c, t, n, r, stats, p_out, st)) return rc;
    }
    c->v.fused_produced(par);
    return seq.ok();
  }
  // the adaptive band (MDR_OPT_GQ_ADAPTIVE): the band is predicted from the crossing's
  // trend, so a budget whose change departs from the last change by more than four superbins' worth of
  // power (a regular-steps edge, the tick after it) would miss it — that tick runs the three-launch
  // form (bins -> compact -> select, cheaper than a band miss), decided on the host from the budgets
  double pavg = 0.0;
  for (int k = 0; k < c->cfg.n_cap; ++k) pavg += c->cfg.cap_table[k] / c->cfg.cop;
  pavg /= c->cfg.n_cap > 0 ? c->cfg.n_cap : 1;
  const double jump = 4.0 * ((double)c->kp.n_global * 64.0 / (double)gq_bins_eff(c->kp.n_global)) * pavg;
  Sequence seq(c->v);  // (not a kRollout: every tick's step says what it leaves, and n may be 0)
  for (int t = 0; t < n; ++t) {
    uint8_t* a = action + (int64_t)t * act_stride;
    double* r = reward + (int64_t)t * rew_stride;
    const double sb = ticks[t].s_prev;
    c->gq_band_skip = c->gq_adaptive && c->v.budget_jumps(sb, jump);
    const int rc0 = mdr_ctrl_greedy(c, sb, a, stream);
    c->gq_band_skip = false;
    if (rc0) return rc0;
    c->v.budget_decided(sb);
    if (int rc = launch_step(c, a, MDR_ACT_BUFFER, to_tick(&ticks[t]), nullptr, r, 0, MDR_CTRL_GREEDY_KEYS, nullptr,
                             stats ? c->d_rows_p + t % kTickRowsBatch : p_out, st))
      return rc;
    if (c->kp.penalty_mode != MDR_PEN_INDIVIDUAL_L2) {  // (Environment.step_tensor's common-penalty tail)
      if (int rc = mdr_penalty_partials(c, stream)) return rc;
      if (int rc = mdr_reward_finalize(c, &ticks[t], r, stream)) return rc;
    }
    if (stats)  // the post-step state with this tick's final rewards
      if (int rc = greedy_rows_tick(c, t, n, r, stats, p_out, st)) return rc;
  }
  return seq.ok();
}

int mdr_greedy_rollout(mdr_ctx* c, int n, const mdr_tick* ticks, uint8_t* action, int64_t act_stride,
                       double* reward, int64_t rew_stride, double* p_out, void* stream) {
  if (!c || (n > 0 && (!ticks || !action || !reward))) return fail(MDR_EARG, "mdr_greedy_rollout: null argument");
  if (n < 0 || act_stride < 0 || rew_stride < 0) return fail(MDR_EARG, "mdr_greedy_rollout: negative size");
  if (int rc_ = cluster_ready(c, "mdr_greedy_rollout")) return rc_;
  if (c->world > 1)  // (a shard-local decision and step would use shard-local counts: per-tick loop)
    return fail(MDR_ESTATE, "mdr_greedy_rollout: single-GPU only (sharded contexts: the per-tick greedy + step loop)");
  return greedy_rollout_seq(c, n, ticks, action, act_stride, reward, rew_stride, p_out, nullptr, stream);
}

int mdr_greedy_rollout_stats(mdr_ctx* c, int n, const mdr_tick* ticks, uint8_t* action, int64_t act_stride,
                             double* reward, int64_t rew_stride, double* p_out, double* stats, int row0,
                             void* stream) {
  // (the checks of the plain arguments first: they need no context, so no device either)
  if (n < 0 || act_stride < 0 || rew_stride < 0) return fail(MDR_EARG, "mdr_greedy_rollout_stats: negative size");
  if (row0 < 0) return fail(MDR_EARG, "mdr_greedy_rollout_stats: negative row0");
  if (n > 0 && !stats) return fail(MDR_EARG, "mdr_greedy_rollout_stats: null stats rows (mdr_greedy_rollout writes none)");
  if (!c || (n > 0 && (!ticks || !action || !reward)))
    return fail(MDR_EARG, "mdr_greedy_rollout_stats: null argument");
  if (int rc_ = cluster_ready(c, "mdr_greedy_rollout_stats")) return rc_;
  if (int rc = check_tick_stats_ctx(c, "mdr_greedy_rollout_stats")) return rc;
  if (n == 0) return MDR_OK;
  if (int rc = rows_scratch(c)) return rc;
  return greedy_rollout_seq(c, n, ticks, action, act_stride, reward, rew_stride, p_out,
                            stats + (size_t)row0 * kTickRow, stream);
}

int mdr_greedy_band(mdr_ctx* c, uint64_t* out) {
  if (!c || !out) return fail(MDR_EARG, "mdr_greedy_band: null argument");
  for (int k = 0; k < 4; ++k) out[k] = 0;
  if (!c->g_sel) return MDR_OK;
  unsigned char h[kGqSelBytes];
  HIP_TRY(hipMemcpy(h, c->g_sel, kGqSelBytes, hipMemcpyDeviceToHost));
  gq_band_of(h, out);
  return MDR_OK;
}

int mdr_greedy_fallbacks(mdr_ctx* c, uint64_t* count) {
  if (!c || !count) return fail(MDR_EARG, "mdr_greedy_fallbacks: null argument");
  uint64_t d[4];
  if (int rc = mdr_greedy_diag(c, d)) return rc;
  *count = d[0];
  return MDR_OK;
}

// ---- sharded histogram select (the stages between the caller's collectives; mdr.h)
static double greedy_pmin(const mdr_ctx* c) {
  double pmin = INFINITY;
  for (int k = 0; k < c->cfg.n_cap; ++k) pmin = fmin(pmin, c->cfg.cap_table[k] / c->cfg.cop);
  return pmin;
}

int mdr_gq_shard_begin(mdr_ctx* c, void* stream) {
  if (!c) return fail(MDR_EARG, "mdr_gq_shard_begin: null context");
  if (int rc_ = cluster_ready(c, "mdr_gq_shard_begin")) return rc_;
  if (c->kp.n_cap > 4) return fail(MDR_EARG, "mdr_gq_shard_begin: more than 4 capacity classes (use the all-gather form)");
  const bool keys_ready = c->v.take_keys() && c->g_cap >= c->kp.n;
  enter_writer(c);
  Sequence seq(c->v);
  if (int rc = greedy_scratch(c, c->kp.n)) return rc;
  hipStream_t st = S(stream);
  if (!keys_ready)
    if (int rc = launch_gq_keys(c, st, nullptr, false)) return rc;
  hipLaunchKernelGGL(k_gq_range, dim3(1), dim3(256), 0, st, c->g_part, c->v.nparts(), c->g_range);
  LAUNCH_CHECK("k_gq_range");
  return seq.ok();
}

int mdr_gq_shard_buffers(mdr_ctx* c, void** super_hist, int64_t* n_super, void** bin_hist, int64_t* n_bin,
                         void** range, void** window, int64_t* window_bytes) {
  if (!c || !super_hist || !n_super || !bin_hist || !n_bin || !range || !window || !window_bytes)
    return fail(MDR_EARG, "mdr_gq_shard_buffers: null argument");
  if (!c->g_sel) return fail(MDR_ESTATE, "mdr_gq_shard_buffers: call mdr_gq_shard_begin first");
  *super_hist = c->g_hist + kGqBins * 4;
  *n_super = (int64_t)kGqCopies * (kGqSuper + 1) * 4;
  *bin_hist = c->g_hist;
  *n_bin = (int64_t)kGqCopies * 512;
  *range = c->g_range;
  *window = c->g_win;
  *window_bytes = (int64_t)(kGqCap + 1) * (int64_t)sizeof(uint4);
  return MDR_OK;
}

int mdr_gq_shard_bins(mdr_ctx* c, double budget, void* stream) {
  if (!c || !c->g_sel) return fail(MDR_ESTATE, "mdr_gq_shard_bins: call mdr_gq_shard_begin first");
  hipLaunchKernelGGL(k_gq_bins, dim3(kGqParts), dim3(kGqThreads), 0, S(stream), c->kp, gq_codes(c), c->g_hist,
                     budget, c->g_sel, (unsigned long long*)nullptr);
  LAUNCH_CHECK("k_gq_bins (sharded)");
  return MDR_OK;
}

int mdr_gq_shard_compact(mdr_ctx* c, double budget, uint8_t* action, void* stream) {
  if (!c || !action) return fail(MDR_EARG, "mdr_gq_shard_compact: null argument");
  if (!c->g_sel) return fail(MDR_ESTATE, "mdr_gq_shard_compact: call mdr_gq_shard_begin first");
  hipStream_t st = S(stream);
  const int nstage = (int)((c->kp.n + kGqStage - 1) / kGqStage);
  hipLaunchKernelGGL(k_gq_compact, dim3(nstage), dim3(kGqThreads), 0, st, c->kp, gq_codes(c), c->g_hist,
                     budget, c->g_sel, c->g_win + 1, action, (unsigned long long*)nullptr);
  LAUNCH_CHECK("k_gq_compact (sharded)");
  // the window's header {count, 0, 0, 0}: the allocator's final count
  HIP_TRY(hipMemsetAsync(c->g_win, 0, sizeof(uint4), st));
  HIP_TRY(hipMemcpyAsync(c->g_win, reinterpret_cast<const unsigned char*>(c->g_sel) + gq_wcount_offset(),
                         sizeof(unsigned), hipMemcpyDeviceToDevice, st));
  return MDR_OK;
}

int mdr_gq_shard_select(mdr_ctx* c, double budget, const void* gathered, int world, uint8_t* action, void* stream) {
  if (!c || !gathered || !action) return fail(MDR_EARG, "mdr_gq_shard_select: null argument");
  if (world < 1 || world > kGqMaxRanks) return fail(MDR_EARG, "mdr_gq_shard_select: 1 <= world <= 64");
  if (!c->g_sel) return fail(MDR_ESTATE, "mdr_gq_shard_select: call mdr_gq_shard_begin first");
  hipLaunchKernelGGL(k_gq_select, dim3(kGqSelBlocks), dim3(1024), 0, S(stream), c->kp, (const uint4*)nullptr,
                     c->g_sorted, budget, greedy_pmin(c), c->g_sel, action, (unsigned long long*)nullptr, c->g_hist,
                     static_cast<const uint4*>(gathered), world, c->g_tickets, (const double*)c->g_range, -1,
                     c->g_map);
  LAUNCH_CHECK("k_gq_select (sharded)");
  c->v.hist_consumed();
  return MDR_OK;
}

int mdr_gq_shard_fallback(mdr_ctx* c, int* need, void* stream) {
  if (!c || !need) return fail(MDR_EARG, "mdr_gq_shard_fallback: null argument");
  if (!c->g_sel) return fail(MDR_ESTATE, "mdr_gq_shard_fallback: call mdr_gq_shard_begin first");
  unsigned v = 0;
  hipStream_t st = S(stream);
  HIP_TRY(hipMemcpyAsync(&v, reinterpret_cast<const unsigned char*>(c->g_sel) + gq_need_fb_offset(), sizeof(v),
                         hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *need = v ? 1 : 0;
  return MDR_OK;
}

int mdr_rccl_allgather(mdr_ctx* c, const void* send, void* recv, int64_t bytes, void* stream) {
  if (!c || !send || !recv || bytes < 0) return fail(MDR_EARG, "mdr_rccl_allgather: bad argument");
  if (!c->comm) return fail(MDR_ESTATE, "mdr_rccl_allgather: RCCL not initialised");
  RCCL_TRY(ncclAllGather(send, recv, (size_t)bytes, ncclUint8, c->comm, S(stream)));
  return MDR_OK;
}

int mdr_greedy_inputs(mdr_ctx* c, double* key, double* power, uint8_t* lock, void* stream) {
  if (!c || !key || !power || !lock) return fail(MDR_EARG, "mdr_greedy_inputs: null argument");
  if (int rc_ = cluster_ready(c, "mdr_greedy_inputs")) return rc_;
  hipLaunchKernelGGL(k_greedy_inputs, dim3(blocks(c->kp.n, 256)), dim3(256), 0, S(stream), c->kp, key, power, lock);
  LAUNCH_CHECK("k_greedy_inputs");
  return MDR_OK;
}

int mdr_greedy_select(mdr_ctx* c, int64_t n, const double* key, const double* power, const uint8_t* lock,
                      double budget, uint8_t* action, void* stream) {
  if (!c || !key || !power || !lock || !action || n < 1) return fail(MDR_EARG, "mdr_greedy_select: bad argument");
  if (n >= ((int64_t)1 << 31)) return fail(MDR_EARG, "mdr_greedy_select: n must be < 2^31");
  int rc = greedy_scratch(c, n);
  if (rc) return rc;
  hipStream_t st = S(stream);
  hipLaunchKernelGGL(k_greedy_iota, dim3(blocks(n, 256)), dim3(256), 0, st, n, c->g_idx);
  LAUNCH_CHECK("k_greedy_iota");
  size_t b = c->g_tmp.capacity();
  HIP_TRY(greedy_sort(c->g_tmp, b, key, c->g_key2, c->g_idx, c->g_idx2, n, st));
  hipLaunchKernelGGL(k_greedy_gather_rows, dim3(blocks(n, 256)), dim3(256), 0, st, n, c->g_idx2, power, lock,
                     c->g_ps, c->g_ls);
  LAUNCH_CHECK("k_greedy_gather_rows");
  b = c->g_tmp.capacity();
  HIP_TRY(hipcub::DeviceScan::InclusiveSum(c->g_tmp.get(), b, c->g_ps.get(), c->g_incl.get(), (int)n, st));
  double pmin = INFINITY;
  for (int k = 0; k < c->cfg.n_cap; ++k) pmin = fmin(pmin, c->cfg.cap_table[k] / c->cfg.cop);
  hipLaunchKernelGGL(k_greedy_walk, dim3(1), dim3(256), 0, st, n, c->g_incl, c->g_ps, c->g_ls, budget, pmin,
                     c->g_kpos, c->g_extra, 64);
  LAUNCH_CHECK("k_greedy_walk");
  hipLaunchKernelGGL(k_greedy_apply, dim3(blocks(n, 256)), dim3(256), 0, st, n, c->g_idx2, c->g_kpos, c->g_extra,
                     action);
  LAUNCH_CHECK("k_greedy_apply");
  return MDR_OK;
}

// ------------------------------------------------------------------------------------ RCCL
int mdr_rccl_unique_id(uint8_t* id128) {
  if (!id128) return fail(MDR_EARG, "mdr_rccl_unique_id: null");
  ncclUniqueId id;
  RCCL_TRY(ncclGetUniqueId(&id));
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  memcpy(id128, &id, 128);
  return MDR_OK;
}

int mdr_rccl_init(mdr_ctx* c, const uint8_t* id128, int world, int rank) {
  if (!c || !id128 || world < 1 || rank < 0 || rank >= world) return fail(MDR_EARG, "mdr_rccl_init: bad argument");
  if (c->host.allreduce) return fail(MDR_ESTATE, "mdr_rccl_init: the context already has host collectives");
  if (c->batch.n_envs) return fail(MDR_ESTATE, "mdr_rccl_init: the context holds a batch of clusters (one GPU)");
  HIP_TRY(hipSetDevice(c->cfg.device));
  ncclUniqueId id;
  memcpy(&id, id128, 128);
  RCCL_TRY(ncclCommInitRank(&c->comm, world, id, rank));
  if (!c->comm_stream) HIP_TRY(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
  c->world = world;
  c->rank = rank;
  return MDR_OK;
}

int mdr_comm_host(mdr_ctx* c, int world, int rank, mdr_host_allreduce_fn allreduce, mdr_host_sendrecv_fn sendrecv,
                  void* user) {
  if (!c || !allreduce || !sendrecv || world < 1 || rank < 0 || rank >= world)
    return fail(MDR_EARG, "mdr_comm_host: bad argument");
  if (c->comm) return fail(MDR_ESTATE, "mdr_comm_host: the context already has an RCCL communicator");
  if (c->batch.n_envs) return fail(MDR_ESTATE, "mdr_comm_host: the context holds a batch of clusters (one GPU)");
  HIP_TRY(hipSetDevice(c->cfg.device));
  if (!c->comm_stream) HIP_TRY(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
  c->host.allreduce = allreduce;
  c->host.sendrecv = sendrecv;
  c->host.user = user;
  c->world = world;
  c->rank = rank;
  return MDR_OK;
}

int mdr_rccl_allreduce(mdr_ctx* c, void* buf, int64_t count, int dtype, void* stream) {
  if (!c || !buf || count < 0) return fail(MDR_EARG, "mdr_rccl_allreduce: bad argument");
  if (!c->comm) return fail(MDR_ESTATE, "mdr_rccl_allreduce: RCCL not initialised");
  ncclDataType_t t = dtype == 0 ? ncclInt64 : dtype == 3 ? ncclUint32 : ncclFloat64;
  ncclRedOp_t op = dtype == 2 ? ncclMax : dtype == 4 ? ncclMin : ncclSum;
  RCCL_TRY(ncclAllReduce(buf, buf, (size_t)count, t, op, c->comm, S(stream)));
  return MDR_OK;
}

}  // extern "C"

namespace {
// Overlapped sharded pipeline (in-kernel action source with lookahead, one reward row per tick).
// The per-tick exchange only feeds the reward's signal term, so the reward of tick t is written
// one launch later (k_step reward_lag; bit-identical, no extra bytes):
//   compute stream  K(t): state of tick t, reward of tick t-1 from the loaded state + allreduced
//                   slab (t-1)%4, lookahead counts of t+1 into slab (t+1)%4, zero slab (t+2)%4
//   comm stream     allreduce(slab t%4) once K(t-1) has filled it — concurrent with K(t)
// K(t+1) waits for allreduce(t); after the loop k_reward_state writes the last tick's reward.
int rollout_sharded_overlap(mdr_ctx* c, const RolloutArgs& a, hipStream_t st) {
  const TickArgs* ticks = c->d_ticks;
  const int n = a.n, mode = a.mode;
  hipStream_t cs = c->comm_stream;
  auto slab = [&](int t) { return c->d_slab + (size_t)(t % kSlabs) * c->slab_len; };
  HIP_TRY(hipMemsetAsync(c->d_slab, 0, kSlabs * c->slab_len * sizeof(unsigned long long), st));
  if (int rc = launch_counts(c, nullptr, mode, 0, ticks, st, slab(0))) return rc;
  HIP_TRY(hipEventRecord(c->ev_pc, st));
  for (int t = 0; t < n; ++t) {
    // comm stream: counts of tick t are complete once K(t-1) (or phase 1) has finished
    HIP_TRY(hipStreamWaitEvent(cs, t == 0 ? c->ev_pc : c->ev_k1[(t - 1) % kSlabs], 0));
    if (int rc = comm_allreduce(c, slab(t), c->slab_len, 0, cs)) return rc;
    HIP_TRY(hipEventRecord(c->ev_ar[t % kSlabs], cs));
    // compute stream: K(t) needs the allreduced counts of tick t-1 for that tick's reward
    if (t >= 1) HIP_TRY(hipStreamWaitEvent(st, c->ev_ar[(t - 1) % kSlabs], 0));
    int rc = launch_step_on(c, nullptr, mode, TickArgs{}, ticks + t, a.rew_row(t >= 1 ? t - 1 : 0), mode,
                            MDR_CTRL_NONE, nullptr, nullptr, t >= 1 ? slab(t - 1) : nullptr, slab(t + 1),
                            slab(t + 2), 1, st);
    if (rc) return rc;
    c->v.step_issued(true, false, /*keep_ring=*/true);  // (this pipeline's own ring of kSlabs)
    HIP_TRY(hipEventRecord(c->ev_k1[t % kSlabs], st));
  }
  HIP_TRY(hipStreamWaitEvent(st, c->ev_ar[(n - 1) % kSlabs], 0));
  hipLaunchKernelGGL(k_reward_state, dim3(blocks(c->kp.n, 256)), dim3(256), 0, st, c->kp,
                     ticks + (n - 1), slab(n - 1), a.rew_row(n - 1), a.p_out);
  LAUNCH_CHECK("k_reward_state");
  // leave the step path's invariant (slab ring+1 zero) behind
  HIP_TRY(hipMemsetAsync(c->d_slab, 0, kSlabs * c->slab_len * sizeof(unsigned long long), st));
  c->v.slabs_zeroed();
  return MDR_OK;
}

// Serial sharded ticks on one stream: [phase 1 if needed] -> allreduce(counts) -> k_step.
// xpart (mdr_rollout_sharded_stats): every tick's P on the device and mdr_tick_stats' two launches
// behind its step, into this rank's partial row t.
int rollout_sharded_serial(mdr_ctx* c, const RolloutArgs& a, hipStream_t st, double* xpart = nullptr) {
  const TickArgs* ticks = c->d_ticks;
  const int n = a.n, mode = a.mode;
  double* const p_tick = a.p_out ? a.p_out : c->d_stat_p.get();  // (rows: every tick's P, for its row)
  HIP_TRY(hipMemsetAsync(c->d_slab, 0, kSlabs * c->slab_len * sizeof(unsigned long long), st));
  c->v.slabs_zeroed();
  const bool la = lookahead_ok(mode);
  for (int t = 0; t < n; ++t) {
    if (!la || t == 0)
      if (int rc = launch_counts(c, a.act_row(t), mode, 0, ticks + t, st)) return rc;
    if (int rc = comm_allreduce(c, slab_at(c, c->v.ring()), c->slab_len, 0, st)) return rc;
    int rc = launch_step(c, a.act_row(t), mode, TickArgs{}, ticks + t, a.rew_row(t), la ? mode : 0, MDR_CTRL_NONE,
                         nullptr, xpart ? p_tick : t == n - 1 ? a.p_out : nullptr, st);
    if (rc) return rc;
    if (xpart)
      if (int rc2 = launch_tick_stats(c, a.rew_row(t), p_tick, 0.0, xpart + (size_t)t * kTickRow, st)) return rc2;
  }
  return MDR_OK;
}

}  // namespace

extern "C" {

// who writes the stats rows of a sharded rollout from this action source (mdr_rollout_stats_path's
// answers without its single-shard refusal), or why nobody does
static int rollout_sharded_stats_path(mdr_ctx* c, int mode, const std::string& who) {
  if (window_ok(c, mode))
    return fail(MDR_EARG, who + ": no stats rows from the open-loop window rollout (k_step_window); use the "
                                "bang-bang sources, or mdr_set_rollout_window(0) for one launch per tick");
  return closed_ok(c, mode, true) ? MDR_STATS_CLOSED_WINDOWS : MDR_STATS_PER_TICK;
}

int mdr_rollout_sharded_stats_path(mdr_ctx* c, int mode) {
  const char* const who = "mdr_rollout_sharded_stats";
  if (!c) return fail(MDR_EARG, "mdr_rollout_sharded_stats_path: null ctx");
  if (int rc_ = cluster_ready(c, "mdr_rollout_sharded_stats_path")) return rc_;
  if (!has_comm(c)) return fail(MDR_ESTATE, std::string(who) + ": no communicator (mdr_rccl_init / mdr_comm_host)");
  if (!check_mode(mode)) return fail(MDR_EARG, "mdr_rollout_sharded_stats_path: bad action source");
  if (win_common(c)) return fail(MDR_EARG, std::string(who) + ": common penalty modes need the per-step API");
  return rollout_sharded_stats_path(c, mode, who);
}

// (stats == nullptr: mdr_rollout_sharded, launch for launch)
int mdr_rollout_sharded_stats(mdr_ctx* c, int n, const mdr_tick* ticks, const uint8_t* action,
                              int64_t act_stride, int mode, double* reward, int64_t rew_stride, double* p_out,
                              double* stats, int64_t stats_rows, int64_t stats_row0, void* stream) {
  const RolloutArgs a{n, action, act_stride, mode, reward, rew_stride, p_out};
  const char* const who = stats ? "mdr_rollout_sharded_stats" : "mdr_rollout_sharded";
  if (stats)  // (before anything is staged or launched, and before any other answer)
    if (int rc = check_stats_rows(who, n, stats_rows, stats_row0)) return rc;
  // a single window begun by mdr_rollout_begin on this sharded context (count, allreduce, P-only
  // reduce already issued): only the KA step kernel is left, with these drivers as its arguments.
  // (Such a call passes every check of the preamble: mdr_rollout_begin made them.  Never with rows:
  // the open-loop windows write none.)
  const bool counted = !stats && c && ticks && n >= 1 && begun_matches(c, a, ticks, true);
  if (int rc = rollout_preamble(c, who, ticks && reward, a, (counted ? 0 : kDropBegun) | kShardedOnly | kNoCommon))
    return rc;
  hipStream_t st = S(stream);
  if (stats) {
    // the partial rows' path and buffers, reserved outside the launch sequence; then the sequence of
    // mdr_rollout_sharded with the rows' launches in it, and ONE exchange + combine behind it
    const int path = rollout_sharded_stats_path(c, mode, who);
    if (path < 0) return path;
    const bool closed = path == MDR_STATS_CLOSED_WINDOWS;
    if (int rc = stats_exchange_reserve(c, n, who)) return rc;
    if (closed) {
      if (int rc = dev_reserve(c->d_wstat, mdr_window_stats_bytes(c->kp.n) / sizeof(double), "d_wstat")) return rc;
    } else {
      if (!p_out)
        if (int rc = dev_reserve(c->d_stat_p, 1, "d_stat_p")) return rc;
      if (int rc = tick_scratch(c)) return rc;
    }
    Sequence seq(c->v, Sequence::kRollout);
    int rc = refresh_if_dirty(c, st);
    if (!rc) rc = stage_ticks(c, n, ticks, st);
    if (rc) return rc;
    double* const xpart = stats_part_rows(c, n, 0);
    if (closed) {
      rc = wslab_clean(c, st);
      if (rc) return rc;
      const bool pipe = c->win_pipe && c->comm_stream && rew_stride != 0;  // (one shared row: one stream)
      rc = pipe ? closed_sharded_pipeline(c, a, st, xpart) : closed_sharded_serial(c, a, st, xpart);
    } else {
      // (never rollout_sharded_overlap: it writes tick t's reward one launch late)
      rc = rollout_sharded_serial(c, a, st, xpart);
    }
    if (!rc) rc = stats_rows_exchange(c, n, closed, stats + (size_t)stats_row0 * kTickRow, st);
    if (rc) (void)hipMemsetAsync(c->d_xstat, 0, dev_bytes(c->d_xstat), st);  // (the slab's invariant, whatever was written)
    return seq.end(rc);
  }
  Sequence seq(c->v, Sequence::kRollout);
  if (counted) {
    c->v.early_consumed();
    int rc = ensure_ticks(c, n);
    if (!rc) rc = window_launches_direct(c, a, ticks, kBegunAllreduced, st);
    return seq.end(rc);
  }
  int rc = refresh_if_dirty(c, st);
  if (rc) return rc;
  rc = stage_ticks(c, n, ticks, st);
  if (rc) return rc;
  if (window_ok(c, mode)) {
    rc = wslab_clean(c, st);
    if (rc) return rc;
    const bool pipe = c->win_pipe && c->comm_stream && pipe_buffers(c);
    return seq.end(pipe ? window_pipeline(c, a, st) : window_launches(c, a, true, st));
  }
  if (closed_ok(c, mode)) {  // (individual_L2: the preamble refused the common penalty modes)
    rc = wslab_clean(c, st);
    if (rc) return rc;
    const bool pipe = c->win_pipe && c->comm_stream && rew_stride != 0;  // (one shared row: one stream)
    return seq.end(pipe ? closed_sharded_pipeline(c, a, st) : closed_sharded_serial(c, a, st));
  }
  const bool can_overlap = lookahead_ok(mode) && rew_stride != 0 && c->comm_stream;
  if (can_overlap && c->tick_overlap) return seq.end(rollout_sharded_overlap(c, a, st));
  return seq.end(rollout_sharded_serial(c, a, st));
}

int mdr_rollout_sharded(mdr_ctx* c, int n, const mdr_tick* ticks, const uint8_t* action,
                        int64_t act_stride, int mode, double* reward, int64_t rew_stride, double* p_out,
                        void* stream) {
  return mdr_rollout_sharded_stats(c, n, ticks, action, act_stride, mode, reward, rew_stride, p_out, nullptr, 0, 0,
                                   stream);
}

int mdr_rollout_sharded_mode(mdr_ctx* c, int* window_pipeline, int* tick_overlap) {
  if (!c || !window_pipeline || !tick_overlap) return fail(MDR_EARG, "mdr_rollout_sharded_mode: null argument");
  *window_pipeline = c->win > 0 && c->win_pipe && c->comm_stream != nullptr;
  *tick_overlap = c->tick_overlap && c->comm_stream != nullptr;
  return MDR_OK;
}

int mdr_set_rollout_window(mdr_ctx* c, int ticks) {
  enter_writer(c);  // (writes no state; kept as it was: DESIGN §7.2, the sites kept for compatibility)
  if (!c || ticks < 0 || ticks > kWindowMax) return fail(MDR_EARG, "mdr_set_rollout_window: ticks outside 0..32");
  if (ticks > 0 && !c->d_wslab) return fail(MDR_EARG, "mdr_set_rollout_window: more than 4 capacity classes");
  if (ticks != c->win) {
    HIP_TRY(hipDeviceSynchronize());  // cached graphs may be in flight
    destroy_graphs(c);
    c->win = ticks;
  }
  return MDR_OK;
}

int mdr_cluster_stats(mdr_ctx* c, const double* reward, double* out, void* stream) {
  if (!c || !out) return fail(MDR_EARG, "mdr_cluster_stats: null argument");
  if (int rc_ = cluster_ready(c, "mdr_cluster_stats")) return rc_;
  if (int rc = dev_reserve(c->d_stats, (size_t)kStats * kStatsBlocks, "d_stats")) return rc;
  const unsigned nb = (unsigned)std::min<int64_t>(kStatsBlocks, (c->kp.n + 255) / 256);
  hipLaunchKernelGGL(k_cluster_stats, dim3(nb), dim3(256), 0, S(stream), c->kp, reward, c->d_stats);
  LAUNCH_CHECK("k_cluster_stats");
  hipLaunchKernelGGL(k_cluster_stats_final, dim3(1), dim3(64), 0, S(stream), c->d_stats, (int)nb, out);
  LAUNCH_CHECK("k_cluster_stats_final");
  return MDR_OK;
}

int mdr_params_changed(mdr_ctx* c) {
  enter_writer(c);
  if (!c) return fail(MDR_EARG, "mdr_params_changed: null ctx");
  c->v.params_replaced();
  return MDR_OK;
}

// ------------------------------------------------------------------------------------ diagnostics
int mdr_probe_stream(mdr_ctx* c, double* reward, void* stream) {
  enter_writer(c);  // (writes no state; kept as it was: DESIGN §7.2, the sites kept for compatibility)
  if (!c || !reward) return fail(MDR_EARG, "mdr_probe_stream: null argument");
  if (!c->bound) return fail(MDR_ESTATE, "mdr_probe_stream: context not bound");
  hipLaunchKernelGGL(k_probe_stream, dim3(blocks(c->kp.n, 512)), dim3(256), 0, S(stream), c->kp, reward);
  LAUNCH_CHECK("k_probe_stream");
  return MDR_OK;
}

int mdr_div_check(const double* a, const double* b, int64_t n, int64_t* mismatches, void* stream) {
  if (!a || !b || !mismatches || n < 0) return fail(MDR_EARG, "mdr_div_check: bad argument");
  HIP_TRY(hipMemsetAsync(mismatches, 0, sizeof(int64_t), S(stream)));
  hipLaunchKernelGGL(k_div_check, dim3(blocks(n, 256)), dim3(256), 0, S(stream), a, b, n,
                     reinterpret_cast<unsigned long long*>(mismatches));
  LAUNCH_CHECK("k_div_check");
  return MDR_OK;
}

// ------------------------------------------------------------------------------------ events
int mdr_event_record(mdr_ctx* c, int slot, void* stream) {
  if (!c || slot < 0 || slot >= 16) return fail(MDR_EARG, "mdr_event_record: bad slot");
  HIP_TRY(hipEventRecord(c->ev[slot], S(stream)));
  return MDR_OK;
}

int mdr_event_elapsed_ms(mdr_ctx* c, int s0, int s1, float* ms) {
  if (!c || !ms || s0 < 0 || s1 < 0 || s0 >= 16 || s1 >= 16) return fail(MDR_EARG, "mdr_event_elapsed_ms: bad slot");
  HIP_TRY(hipEventSynchronize(c->ev[s1]));
  HIP_TRY(hipEventElapsedTime(ms, c->ev[s0], c->ev[s1]));
  return MDR_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------ actor
namespace {

int align16(int x) { return (x + 15) & ~15; }

// Packed-image offsets, the obs row's slot layout and the LDS plan of k_actor for `nw` waves per
// block (mdr_actor.h ActorDims).
// the fused kernel's PREC for the loaded actor: 1 bf16, 3 bf16x3, fp32: 4 (the fp16 split, default) or
// 6 (the three-way bf16 split, MDR_OPT_ACTOR_FP32_FORM)
int actor_kprec(const mdr_ctx* c) {
  const int p = c->actor.precision;
  return p == MDR_PREC_BF16 ? 1 : p == MDR_PREC_FP32 ? (c->actor_fp32_bf16 ? 6 : 4) : 3;
}

ActorDims actor_layout(const mdr_actor_spec& a, const mdr_obs_spec* sp, int nw, int kprec) {
  ActorDims d{};
  d.n_in = a.n_in; d.h1 = a.h1; d.h2 = a.h2; d.n_act = a.n_act;
  const int mbn = (std::max(a.h1, a.h2) + kActorRB - 1) / kActorRB;
  d.mb = mbn <= 7 ? 7 : 8;  // (the kernel's instantiations)
  d.nf = kprec == 6 ? 3 : 2;
  d.f16 = kprec == 4;
  const int K = sp->n_comm, M = mdr_msg_width(sp);
  d.n_comm = K;
  d.msg_w = M;
  d.n_own = a.n_in - K * M;
  d.own4 = (d.n_own + 3) & ~3;
  d.m4 = (M + 3) & ~3;
  d.ring = sp->comm_mode == MDR_COMM_RING && K > 0;
  d.lo = d.ring ? K / 2 : 0;
  d.nslot = d.own4 + K * d.m4;
  d.ks1 = std::max(2, (d.nslot + 31) / 32);  // (the kernel's instantiations: 2, 3, 4; a padding k-step is zero)
  int rs = d.ring ? d.m4 + d.own4 : d.nslot;
  if (((rs / 4) & 1) == 0) rs += 4;  // odd multiple of 16 B: conflict-free ds_read_b128 of 16 rows
  d.rs = rs;
  d.nrows = d.ring ? d.lo + 32 + (K + 1) / 2 : 32;
  d.off_w1 = 0;
  d.off_w2 = d.mb * d.ks1 * d.nf * 1024;
  d.off_tail = d.off_w2 + d.mb * kActorKS2 * d.nf * 1024;
  d.off_end = align16(d.off_tail + kActorTailEnd * 4);
  d.lds_cf = d.off_end;
  d.lds_hist = d.lds_cf + align16(kObsConst * 4);
  d.lds_b1 = d.lds_hist + MDR_MAX_CAP * 4;
  d.lds_wave = d.lds_b1 + (d.f16 ? 2 * kActorRows * 4 + 16 : 0);  // (b1, b2, max of the fp16 split: mdr_actor.hip)

  d.w_zero = align16(d.nrows * rs * 4);
  d.w_hw = d.w_zero + 16;
  d.w_cls = d.w_hw + 32 * 4;
  d.wave_stride = align16(d.w_cls + 32);
  d.lds_total = d.lds_wave + nw * d.wave_stride;
  return d;
}

// the obs layout k_actor<..., DEF = true> fixes at compile time: the reference's defaults (the
// 'neighbours' ring, messages of 4 features, no hvac / solar / thermal state features), <= 64 slots, rows of 20 floats
bool actor_def_layout(const mdr_ctx* c, const mdr_obs_spec* sp, const ActorDims& d) {
  return !c->actor_generic && sp->comm_mode == MDR_COMM_RING && sp->n_comm > 0 && !sp->hvac_state && !sp->solar_state &&
         !sp->thermal_state && !sp->msg_thermal && !sp->msg_hvac && d.ring && d.msg_w == 4 && d.n_own == 10 &&
         d.ks1 == 2 && d.rs == 20;
}

int actor_plan(const mdr_ctx* c, const mdr_obs_spec* sp, ActorDims* d, int* nw) {
  const int prec = actor_kprec(c);
  *d = actor_layout(c->actor, sp, 1, prec);
  if (d->n_own < 0 || d->nslot > kActorMaxSlots)
    return fail(MDR_EARG, "mdr_actor: obs row wider than the actor's 128 feature slots");
  for (int w = actor_max_waves(prec, actor_def_layout(c, sp, *d)); w >= 1; --w) {
    *d = actor_layout(c->actor, sp, w, prec);
    d->w1raw = c->d_actor_raw;
    if (d->lds_total <= 160 * 1024) { *nw = w; return MDR_OK; }
  }
  return fail(MDR_EARG, "mdr_actor: weights + obs rows exceed the 160 KiB LDS of a CU");
}

// the loaded net takes the fused k_actor for this obs layout (two hidden layers <= 128 wide, the obs
// row within 128 slots, weights + rows within the LDS); otherwise the chain runs it
bool actor_fused_ok(const mdr_ctx* c, const mdr_obs_spec* sp) {
  const mdr_actor_net& a = c->net;
  if (a.n_hidden != 2 || a.hidden[0] > kActorRows || a.hidden[1] > kActorRows || a.n_in > kActorMaxIn) return false;
  ActorDims d;
  int nw = 0;
  const std::string keep = g_err;
  const bool ok = actor_plan(c, sp, &d, &nw) == MDR_OK;
  g_err = keep;
  return ok;
}

// offsets of layer l's weights in the loaded fp32 image [w0 b0 w1 b1 ... wL bL]
size_t net_w_off(const mdr_actor_net& a, int l) {
  size_t o = 0;
  int in = a.n_in;
  for (int k = 0; k < l; ++k) {
    const int out = k < a.n_hidden ? a.hidden[k] : a.n_act;
    o += (size_t)out * in + out;
    in = out;
  }
  return o;
}
int net_width(const mdr_actor_net& a) {
  int w = 0;
  for (int l = 0; l < a.n_hidden; ++l) w = std::max(w, a.hidden[l]);
  return w;
}

// the chain's row buffers for n houses and an F-feature obs row (allocated before any capture)
int chain_ensure(mdr_ctx* c, int F, hipStream_t st) {
  const size_t w4 = (size_t)((net_width(c->net) + 3) & ~3);
  const size_t need = ((size_t)F + 2 * w4) * (size_t)c->kp.n * sizeof(float);
  if (need <= dev_bytes(c->d_chain)) return MDR_OK;
  HIP_TRY(hipStreamSynchronize(st));
  drop_actor_graphs(c);
  return dev_reserve(c->d_chain, need / sizeof(float), "d_chain");
}

// The packed weight image for this obs layout (k_actor_pack from the loaded fp32 weights): packed
// again only when the slot layout or the precision changes.  Called by every actor entry point
// before it launches or captures anything.  (The chain needs no packing: its row buffers.)
int actor_ensure_packed(mdr_ctx* c, const mdr_obs_spec* sp, hipStream_t st) {
  if (!actor_fused_ok(c, sp)) return chain_ensure(c, sp->n_feat, st);
  ActorDims d;
  int nw = 0;
  if (int rc = actor_plan(c, sp, &d, &nw)) return rc;
  const std::vector<int> key{d.n_own, d.own4, d.msg_w, d.m4, d.n_comm, d.mb, d.ks1, d.nf, d.ring, d.lo,
                             c->actor.precision, d.f16};
  if (key == c->actor_key) return MDR_OK;
  if ((size_t)d.off_end > c->d_actor.capacity()) {
    HIP_TRY(hipStreamSynchronize(st));
    drop_actor_graphs(c);
    c->actor_key.clear();  // (no image until k_actor_pack below has one to write)
    if (int rc = dev_reserve(c->d_actor, d.off_end, "d_actor")) return rc;
  }
  const mdr_actor_spec& a = c->actor;
  const float* w1 = c->d_actor_raw;
  const float* b1 = w1 + (size_t)a.h1 * a.n_in;
  const float* w2 = b1 + a.h1;
  const float* b2 = w2 + (size_t)a.h2 * a.h1;
  const float* w3 = b2 + a.h2;
  const float* b3 = w3 + (size_t)kActorNA * a.h2;
  ActorFold fo{};
  if (d.f16) {  // the folded features (mdr_actor.h ActorFold) and bounds on their values (obs_consts)
    int off[3], mk[3];
    int u = obs_uniform_own(sp->hvac_state, sp->solar_state, sp->thermal_state, fo.feat, fo.cf);
    fo.nu_own = u;
    const int um = obs_uniform_msg(sp->msg_thermal, sp->msg_hvac, off, mk);
    for (int k = 0; k < d.n_comm; ++k)
      for (int j = 0; j < um && u < kActorMaxU; ++j) {
        fo.feat[u] = d.n_own + k * d.msg_w + off[j];
        fo.cf[u++] = mk[j];
      }
    fo.nu = u;
    double pmax = 0.0;
    for (int k = 0; k < c->cfg.n_cap; ++k) pmax = std::max(pmax, fabs(c->cfg.cap_table[k] / c->cfg.cop));
    const double R = sp->norm_reg_sig != 0.0 ? fabs(sp->norm_reg_sig) : 1.0;
    for (int j = 0; j < u; ++j) {
      const int k = fo.cf[j];
      // P / R <= n_global P_on,max / R (every house on); the signal, solar, deadband and OD features
      // are O(1) after norm.py's scaling (64 is a bound for the scale choice only: a value beyond it
      // is still exact, k_actor's range check sends its tile to the fp32 fallback)
      const double b = k == 3 ? (double)c->kp.n_global * pmax / R : k <= 2 ? 1.0 : k == 8 ? fabs(c->cfg.cop)
                       : k == 9 ? fabs(c->cfg.lcf) : k == 10 ? fabs(sp->cfg_cap) : 64.0;
      fo.cfmax[j] = (float)std::min(b, 3.0e38);
    }
  }
  const int nthreads = (d.mb * (d.ks1 + kActorKS2) + 1) * 64;
  hipLaunchKernelGGL(k_actor_pack, dim3(blocks(nthreads, 256)), dim3(256), 0, st, d, fo, w1, b1, w2, b2, w3, b3,
                     c->d_actor);
  LAUNCH_CHECK("k_actor_pack");
  c->actor_key = key;
  return MDR_OK;
}

#define MDR_ACTOR_KERNELS_D(MB, KS, D)                                                                 \
  (const void*)k_actor<1, false, MB, KS, D>, (const void*)k_actor<3, false, MB, KS, D>,                   \
      (const void*)k_actor<4, false, MB, KS, D>, (const void*)k_actor<6, false, MB, KS, D>,               \
      (const void*)k_actor<1, true, MB, KS, D>, (const void*)k_actor<3, true, MB, KS, D>,                 \
      (const void*)k_actor<4, true, MB, KS, D>, (const void*)k_actor<6, true, MB, KS, D>
#define MDR_ACTOR_KERNELS(MB, KS) MDR_ACTOR_KERNELS_D(MB, KS, false)


// The general actor as a chain of launches (mdr_actor.hip "chain"): obs rows (into out.obs when the
// caller keeps them), one k_dense per hidden layer (ping-pong row buffers), k_actor_head.
int launch_actor_chain(mdr_ctx* c, const mdr_obs_spec* sp, const ObsArgs& o, const double* p_dev, uint64_t tick,
                       const TickArgs* tkp, const ActorOut& out_in, hipStream_t st) {
  if (out_in.prof) return fail(MDR_EARG, "mdr_actor_profile: the chained actor has no phase profile");
  ActorOut out = out_in;
  out.head = c->actor_head;  // (mdr_actor_set_head)
  out.eps = c->d_eps;
  const mdr_actor_net& a = c->net;
  const int64_t n = c->kp.n;
  const int F = sp->n_feat;
  const int w4 = (net_width(a) + 3) & ~3;
  float* x0 = out.obs ? out.obs : c->d_chain;
  float* hb[2] = {c->d_chain + (size_t)F * n, c->d_chain + ((size_t)F + w4) * n};
  const int lo = sp->n_comm / 2, hi = (sp->n_comm + 1) / 2;
  const size_t tile = ((size_t)kObsBlock * F + 3) & ~(size_t)3;
  const size_t bytes = (tile + (size_t)(lo + kObsBlock + hi) * o.msg_w) * sizeof(float);
  if (bytes > 160 * 1024) return fail(MDR_EARG, "mdr_actor: obs row too wide for one LDS tile");
  hipLaunchKernelGGL(k_obs, dim3(blocks(n, kObsBlock)), dim3(kObsBlock), bytes, st, c->kp, o, p_dev, x0);
  LAUNCH_CHECK("k_obs (actor chain)");
  const float* x = x0;
  int ld = F, K = F;
  const float* raw = c->d_actor_raw;
  const int prec = a.precision;
  for (int l = 0; l < a.n_hidden; ++l) {
    const int out_w = a.hidden[l];
    const float* W = raw + net_w_off(a, l);
    const float* b = W + (size_t)out_w * K;
    float* y = hb[l & 1];
    const dim3 grid(blocks(n, 64), blocks(out_w, 64));
    if (prec == MDR_PREC_BF16) hipLaunchKernelGGL(k_dense<1>, grid, dim3(256), 0, st, x, ld, K, n, W, b, out_w, y, w4, 1);
    else if (prec == MDR_PREC_FP32) hipLaunchKernelGGL(k_dense<6>, grid, dim3(256), 0, st, x, ld, K, n, W, b, out_w, y, w4, 1);
    else hipLaunchKernelGGL(k_dense<3>, grid, dim3(256), 0, st, x, ld, K, n, W, b, out_w, y, w4, 1);
    LAUNCH_CHECK("k_dense");
    x = y;
    ld = w4;
    K = out_w;
  }
  const float* W3 = raw + net_w_off(a, a.n_hidden);
  hipLaunchKernelGGL(k_actor_head, dim3(blocks(n, 256)), dim3(256), 0, st, c->kp, x, ld, K, W3, W3 + (size_t)kActorNA * K,
                     tick, tkp, out);
  LAUNCH_CHECK("k_actor_head");
  return MDR_OK;
}

int launch_actor(mdr_ctx* c, const mdr_obs_spec* sp, const ObsArgs& o, const double* p_dev, uint64_t tick,
                 const TickArgs* tkp, const ActorOut& out_in, hipStream_t st) {
  if (!actor_fused_ok(c, sp)) return launch_actor_chain(c, sp, o, p_dev, tick, tkp, out_in, st);
  ActorOut out = out_in;
  out.ovf = reinterpret_cast<unsigned*>(c->d_flags.get()) + 1;  // (mdr_actor_status; read by the fp16 form only)
  out.head = c->actor_head;  // (mdr_actor_set_head)
  out.eps = c->d_eps;
  ActorDims d;
  int nw = 0;
  if (int rc = actor_plan(c, sp, &d, &nw)) return rc;
  const int64_t ntile_all = (c->kp.n + 31) / 32;
  const int64_t nv = out.tiles == 1 ? ntile_all - 2 : out.tiles == 2 ? 2 : ntile_all;  // (ActorOut.tiles)
  const int64_t ntile = (nv + nw - 1) / nw;  // blocks with at least one tile per wave
  const int64_t cap = c->actor_grid > 0 ? std::min(c->actor_grid, c->n_cu) : c->n_cu;  // (MDR_OPT_ACTOR_GRID)
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ntile, cap));
  static bool lds_attr = false;  // > 64 KiB of dynamic LDS must be opted into per kernel
  if (!lds_attr) {
    for (const void* k : {MDR_ACTOR_KERNELS(7, 2), MDR_ACTOR_KERNELS(7, 3), MDR_ACTOR_KERNELS(7, 4),
                          MDR_ACTOR_KERNELS(8, 2), MDR_ACTOR_KERNELS(8, 3), MDR_ACTOR_KERNELS(8, 4),
                          MDR_ACTOR_KERNELS_D(7, 2, true), MDR_ACTOR_KERNELS_D(8, 2, true)})
      HIP_TRY(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    lds_attr = true;
  }
#define MDR_LAUNCH_ACTOR_S(P, F, MB, KS)                                                                     \
  hipLaunchKernelGGL((k_actor<P, F, MB, KS, false>), dim3(grid), dim3(64 * nw), d.lds_total, st, c->kp, o, d, p_dev, \
                     c->d_actor, out, tick, tkp)
#define MDR_LAUNCH_ACTOR_DEF(P, F, MB)                                                                        \
  hipLaunchKernelGGL((k_actor<P, F, MB, 2, true>), dim3(grid), dim3(64 * nw), d.lds_total, st, c->kp, o, d, p_dev, \
                     c->d_actor, out, tick, tkp)
  const bool def = actor_def_layout(c, sp, d);
#define MDR_LAUNCH_ACTOR(P, F)                                 \
  do {                                                         \
    if (def && d.mb == 7) MDR_LAUNCH_ACTOR_DEF(P, F, 7);         \
    else if (def) MDR_LAUNCH_ACTOR_DEF(P, F, 8);                 \
    else if (d.mb == 7 && d.ks1 == 2) MDR_LAUNCH_ACTOR_S(P, F, 7, 2); \
    else if (d.mb == 7 && d.ks1 == 3) MDR_LAUNCH_ACTOR_S(P, F, 7, 3); \
    else if (d.mb == 7) MDR_LAUNCH_ACTOR_S(P, F, 7, 4);          \
    else if (d.ks1 == 2) MDR_LAUNCH_ACTOR_S(P, F, 8, 2);         \
    else if (d.ks1 == 3) MDR_LAUNCH_ACTOR_S(P, F, 8, 3);         \
    else MDR_LAUNCH_ACTOR_S(P, F, 8, 4);                         \
  } while (0)
  const int prec = actor_kprec(c);
  // the fp16-split form defers a wave's out-of-range tiles to its fallback pass through a 64-bit mask:
  // one launch per 64 tiles of a wave (the same grid: launch k covers the virtual tiles [64 k grid nw,
  // 64 (k + 1) grid nw), ActorOut.tiles bits 2 and up; one launch up to 64 n_cu nw tiles, 6.3M houses
  // on 256 CUs at 12 waves).  The phase profile holds the last launch's waves.
  const int64_t per = 64 * (int64_t)grid * nw;
  const int nlaunch = prec == 4 ? (int)std::max<int64_t>(1, (nv + per - 1) / per) : 1;
  for (int k = 0; k < nlaunch; ++k) {
    out.tiles = out_in.tiles | (k << 2);
    if (out.prof) {
      if (prec == 1) MDR_LAUNCH_ACTOR(1, true);
      else if (prec == 4) MDR_LAUNCH_ACTOR(4, true);
      else if (prec == 6) MDR_LAUNCH_ACTOR(6, true);
      else MDR_LAUNCH_ACTOR(3, true);
    } else {
      if (prec == 1) MDR_LAUNCH_ACTOR(1, false);
      else if (prec == 4) MDR_LAUNCH_ACTOR(4, false);
      else if (prec == 6) MDR_LAUNCH_ACTOR(6, false);
      else MDR_LAUNCH_ACTOR(3, false);
    }
  }
#undef MDR_LAUNCH_ACTOR
#undef MDR_LAUNCH_ACTOR_S
#undef MDR_LAUNCH_ACTOR_DEF
  LAUNCH_CHECK("k_actor");
  return MDR_OK;
}

// the spec is valid for the loaded actor; the weights are packed for its slot layout (before any
// launch or graph capture of the caller)
int check_actor_obs(mdr_ctx* c, const mdr_obs_spec* sp, const char* who, hipStream_t st) {
  if (!c->actor_ready) return fail(MDR_ESTATE, std::string(who) + ": no actor loaded (mdr_actor_load)");
  if (int rc = check_obs_spec(sp, who)) return rc;
  if (sp->n_feat != c->actor.n_in) return fail(MDR_EARG, std::string(who) + ": obs n_feat != actor n_in");
  return actor_ensure_packed(c, sp, st);
}

}  // namespace

extern "C" {

int mdr_actor_load_net(mdr_ctx* c, const mdr_actor_net* a, const float* const* w, const float* const* b,
                       void* stream) {
  if (!c || !a || !w || !b) return fail(MDR_EARG, "mdr_actor_load_net: null argument");
  if (a->n_in < 1 || a->n_in > 4096 || a->n_hidden < 1 || a->n_hidden > MDR_ACTOR_MAX_LAYERS || a->n_act != kActorNA)
    return fail(MDR_EARG, "mdr_actor_load_net: shape outside 1 <= n_in <= 4096, 1..8 hidden layers, n_act == 2");
  for (int l = 0; l < a->n_hidden; ++l)
    if (a->hidden[l] < 1 || a->hidden[l] > 4096) return fail(MDR_EARG, "mdr_actor_load_net: hidden width outside 1..4096");
  if (a->precision != MDR_PREC_BF16 && a->precision != MDR_PREC_BF16X3 && a->precision != MDR_PREC_FP32)
    return fail(MDR_EARG, "mdr_actor_load_net: bad precision");
  for (int l = 0; l <= a->n_hidden; ++l)
    if (!w[l] || !b[l]) return fail(MDR_EARG, "mdr_actor_load_net: null layer");
  // the fp32 weights, kept on device: the fused kernel's packed image depends on the obs layout, so
  // it is made by the first actor call of each layout (actor_ensure_packed)
  const size_t nraw = net_w_off(*a, a->n_hidden + 1);
  // captured actor graphs hold the chain's weight pointers and the fused / chain choice: they stay
  // valid while the buffer and the net's shape do (a PPO update reloads weights of the same shape)
  const bool same = c->actor_ready && memcmp(&c->net, a, sizeof(mdr_actor_net)) == 0;
  if (!same || nraw > c->d_actor_raw.capacity()) drop_actor_graphs(c);
  if (nraw > c->d_actor_raw.capacity()) {
    HIP_TRY(hipStreamSynchronize(S(stream)));
    c->actor_ready = false;  // (no weights until the copies below are queued)
    if (int rc = dev_reserve(c->d_actor_raw, nraw, "d_actor_raw")) return rc;
  }
  float* r = c->d_actor_raw;
  int in = a->n_in;
  for (int l = 0; l <= a->n_hidden; ++l) {
    const int out = l < a->n_hidden ? a->hidden[l] : a->n_act;
    HIP_TRY(hipMemcpyAsync(r, w[l], (size_t)out * in * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
    r += (size_t)out * in;
    HIP_TRY(hipMemcpyAsync(r, b[l], (size_t)out * sizeof(float), hipMemcpyDeviceToDevice, S(stream)));
    r += out;
    in = out;
  }
  c->actor_key.clear();
  c->net = *a;
  c->actor = mdr_actor_spec{a->n_in, a->hidden[0], a->n_hidden > 1 ? a->hidden[1] : 0, a->n_act, a->precision};
  c->actor_ready = true;
  return MDR_OK;
}

int mdr_actor_load(mdr_ctx* c, const mdr_actor_spec* a, const float* w1, const float* b1, const float* w2,
                   const float* b2, const float* w3, const float* b3, void* stream) {
  if (!c || !a || !w1 || !b1 || !w2 || !b2 || !w3 || !b3) return fail(MDR_EARG, "mdr_actor_load: null argument");
  mdr_actor_net net{};
  net.n_in = a->n_in;
  net.n_hidden = 2;
  net.n_act = a->n_act;
  net.precision = a->precision;
  net.hidden[0] = a->h1;
  net.hidden[1] = a->h2;
  const float* w[3] = {w1, w2, w3};
  const float* b[3] = {b1, b2, b3};
  return mdr_actor_load_net(c, &net, w, b, stream);
}

int mdr_actor_set_head(mdr_ctx* c, int head, float epsilon, void* stream) {
  if (!c) return fail(MDR_EARG, "mdr_actor_set_head: null context");
  if (head != MDR_HEAD_SOFTMAX && head != MDR_HEAD_Q) return fail(MDR_EARG, "mdr_actor_set_head: unknown head");
  if (!(epsilon >= 0.f && epsilon <= 1.f)) return fail(MDR_EARG, "mdr_actor_set_head: epsilon outside [0, 1]");
  hipLaunchKernelGGL(k_actor_eps, dim3(1), dim3(64), 0, S(stream), c->d_eps, epsilon);
  LAUNCH_CHECK("k_actor_eps");
  c->actor_head = head;
  return MDR_OK;
}

int mdr_actor_status(mdr_ctx* c, int64_t* out, int n, void* stream) {
  if (!c || !out || n < 3) return fail(MDR_EARG, "mdr_actor_status: need out[3]");
  unsigned v[2] = {0u, 0u};
  HIP_TRY(hipStreamSynchronize(S(stream)));
  HIP_TRY(hipMemcpy(v, c->d_flags + 1, sizeof(v), hipMemcpyDeviceToHost));
  const unsigned z[2] = {0u, 0u};
  HIP_TRY(hipMemcpy(c->d_flags + 1, z, sizeof(z), hipMemcpyHostToDevice));
  out[0] = (int64_t)v[0];
  out[1] = c->actor_ready ? actor_kprec(c) : 0;
  out[2] = (int64_t)v[1];
  return MDR_OK;
}

int mdr_actor_fused(mdr_ctx* c, const mdr_obs_spec* sp) {
  if (!c || !sp) return fail(MDR_EARG, "mdr_actor_fused: null argument");
  if (!c->actor_ready) return fail(MDR_ESTATE, "mdr_actor_fused: no actor loaded");
  return actor_fused_ok(c, sp) ? 1 : 0;
}

int mdr_actor_act(mdr_ctx* c, const mdr_obs_spec* sp, const mdr_obs_scalars* sc, const double* p_dev,
                  uint64_t tick, uint8_t* action, float* prob, float* probs, float* obs_out, int count_next,
                  void* stream) {
  enter_writer(c);
  if (!c || !sp || !sc) return fail(MDR_EARG, "mdr_actor_act: null argument");
  if (int rc_ = cluster_ready(c, "mdr_actor_act")) return rc_;
  if (int rc = check_actor_obs(c, sp, "mdr_actor_act", S(stream))) return rc;
  hipStream_t st = S(stream);
  Sequence seq(c->v);
  ActorOut out{action, prob, probs, obs_out, nullptr, nullptr};
  if (count_next) {
    // the counts of the tick these actions drive go into the current slab (from zero)
    out.count_next = slab_at(c, c->v.ring());
    HIP_TRY(hipMemsetAsync(out.count_next, 0, c->slab_len * sizeof(unsigned long long), st));
  }
  if (int rc = launch_actor(c, sp, obs_args(c, sp, sc), p_dev, tick, nullptr, out, st)) return rc;
  if (count_next) c->v.counts_produced();
  return seq.ok();
}

int mdr_actor_profile(mdr_ctx* c, const mdr_obs_spec* sp, const mdr_obs_scalars* sc, const double* p_dev,
                      double* cycles_out, void* stream) {
  if (!c || !sp || !sc || !cycles_out) return fail(MDR_EARG, "mdr_actor_profile: null argument");
  if (int rc_ = cluster_ready(c, "mdr_actor_profile")) return rc_;
  if (int rc = check_actor_obs(c, sp, "mdr_actor_profile", S(stream))) return rc;
  hipStream_t st = S(stream);
  const int nb = c->n_cu * 16;  // waves (at most 16 per block, one block per CU)
  Dev<unsigned long long> d;
  if (int rc = dev_reserve(d, (size_t)nb * 8, "mdr_actor_profile: cycles")) return rc;
  HIP_TRY(hipMemsetAsync(d, 0, (size_t)nb * 8 * sizeof(unsigned long long), st));
  ActorOut out{nullptr, nullptr, nullptr, nullptr, nullptr, d};
  int rc = launch_actor(c, sp, obs_args(c, sp, sc), p_dev, 0, nullptr, out, st);
  std::vector<unsigned long long> h((size_t)nb * 8);
  if (!rc && hipStreamSynchronize(st) == hipSuccess &&
      hipMemcpy(h.data(), d, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
    int used = 0;
    for (int k = 0; k < 8; ++k) cycles_out[k] = 0.0;
    for (int b = 0; b < nb; ++b) {
      if (h[b * 8 + 7] == 0) continue;
      ++used;
      for (int k = 0; k < 8; ++k) cycles_out[k] += (double)h[b * 8 + k];
    }
    for (int k = 0; k < 8; ++k) cycles_out[k] /= used ? used : 1;
  } else if (!rc) {
    rc = fail(MDR_EHIP, "mdr_actor_profile: readback");
  }
  return rc;
}

// ---- per-tick stats rows (k_tick_stats + k_tick_stats_finish): scratch, checks, the two launches
// the block partials belong to the context: allocated (zeroed) before any capture that uses them;
// every launch overwrites the partials it then reads, so no node ever has to clear them
static int tick_scratch(mdr_ctx* c) {
  return dev_reserve(c->d_tick_part, (size_t)kStats * kTickBlocks, "d_tick_part", true);
}

// mdr_greedy_rollout_stats' slabs: a batch of kTickRowsBatch ticks' block partials and cluster powers
static int rows_scratch(mdr_ctx* c) {
  if (int rc = dev_reserve(c->d_rows_part, (size_t)kStats * kTickBlocks * kTickRowsBatch, "d_rows_part", true)) return rc;
  return dev_reserve(c->d_rows_p, kTickRowsBatch, "d_rows_p", true);
}

static int check_tick_stats_ctx(mdr_ctx* c, const char* who) {
  if (has_comm(c) || c->world > 1)
    return fail(MDR_ESTATE, std::string(who) + ": stats rows are single-shard (a row sums this shard's houses only)");
  return MDR_OK;
}

// k_tick_stats over the bound state (+ reward) into partial[nb][kStats]; the instantiation follows
// the pointers' alignment (mdr_kernels.hip)
static int launch_tick_partials(mdr_ctx* c, const double* reward, double* partial, unsigned* nb_out, hipStream_t st) {
  const unsigned nb = std::max(1u, std::min(blocks(blocks(c->kp.n, kTickHpt), kTickBlock), (unsigned)kTickBlocks));
  const KParams& k = c->kp;
  const bool vs = (((uintptr_t)k.t_air | (uintptr_t)k.t_mass | (uintptr_t)k.target | (uintptr_t)k.hvac) & 15) == 0;
  const bool vr = reward && ((uintptr_t)reward & 15) == 0;
#define MDR_LAUNCH_TICK(R, VS, VR) \
  hipLaunchKernelGGL((k_tick_stats<R, VS, VR>), dim3(nb), dim3(kTickBlock), 0, st, c->kp, reward, partial)
  if (!reward) { if (vs) MDR_LAUNCH_TICK(false, true, false); else MDR_LAUNCH_TICK(false, false, false); }
  else if (vs) { if (vr) MDR_LAUNCH_TICK(true, true, true); else MDR_LAUNCH_TICK(true, true, false); }
  else { if (vr) MDR_LAUNCH_TICK(true, false, true); else MDR_LAUNCH_TICK(true, false, false); }
#undef MDR_LAUNCH_TICK
  LAUNCH_CHECK("k_tick_stats");
  *nb_out = nb;
  return MDR_OK;
}

static int launch_tick_stats(mdr_ctx* c, const double* reward, const double* p_dev, double p_host, double* row,
                             hipStream_t st) {
  unsigned nb = 0;
  if (int rc = launch_tick_partials(c, reward, c->d_tick_part, &nb, st)) return rc;
  hipLaunchKernelGGL(k_tick_stats_finish, dim3(1), dim3(kTickBlock), 0, st, c->d_tick_part, (int)nb, p_dev, p_host, row);
  LAUNCH_CHECK("k_tick_stats_finish");
  return MDR_OK;
}

int mdr_tick_stats(mdr_ctx* c, const double* reward, const double* p_dev, double p_host, double* out16,
                   void* stream) {
  if (!out16) return fail(MDR_EARG, "mdr_tick_stats: null out16");
  if (!c) return fail(MDR_EARG, "mdr_tick_stats: null ctx");
  if (int rc_ = cluster_ready(c, "mdr_tick_stats")) return rc_;
  if (int rc = check_tick_stats_ctx(c, "mdr_tick_stats")) return rc;
  if (int rc = tick_scratch(c)) return rc;
  return launch_tick_stats(c, reward, p_dev, p_host, out16, S(stream));
}

// ---- stats rows on a house-sharded cluster: the exchange slab, the partial rows
// and the one exchange + combine per call.  The entry points above keep their single-shard refusals.
static bool ctx_sharded(const mdr_ctx* c);

// the slab's world and this rank's place in it: the communicator's, or what mdr_stats_exchange_ranks
// told a shard whose exchanges are driven by the caller
static int x_world(const mdr_ctx* c) { return has_comm(c) ? c->world : c->x_world > 0 ? c->x_world : 1; }
static int x_rank(const mdr_ctx* c) { return has_comm(c) ? c->rank : c->x_world > 0 ? c->x_rank : 0; }

static int check_stats_rows(const char* who, int64_t n, int64_t stats_rows, int64_t stats_row0) {
  if (stats_rows < 0 || stats_row0 < 0 || n < 0 || stats_row0 > stats_rows - n)
    return fail(MDR_EARG, std::string(who) + ": stats_row0 .. stats_row0 + n_ticks outside [0, stats_rows)");
  return MDR_OK;
}

size_t mdr_stats_exchange_bytes(int world, int m) {
  if (world < 1 || m < 1) return 0;
  const size_t lim = SIZE_MAX / (sizeof(double) * kTickRow);
  if ((size_t)world > lim / (size_t)m) return 0;
  return (size_t)world * (size_t)m * kTickRow * sizeof(double);
}

// room for an m-row call, grown outside any launch sequence: a queued combine may still read and zero
// the old slab, so the device is idle before it is freed; a new slab is zero-filled (the invariant)
static int stats_exchange_reserve(mdr_ctx* c, int m, const char* who) {
  if (!has_comm(c) && c->x_world < 1 && c->kp.n < c->kp.n_global)
    return fail(MDR_ESTATE, std::string(who) + ": a shard without a communicator: mdr_stats_exchange_ranks first");
  const size_t need = mdr_stats_exchange_bytes(x_world(c), m) / sizeof(double);
  if (!need) return fail(MDR_EARG, std::string(who) + ": m outside 1 .. the exchange slab's limit");
  if (need <= c->d_xstat.capacity()) return MDR_OK;
  HIP_TRY(hipDeviceSynchronize());
  return dev_reserve(c->d_xstat, need, "d_xstat", true);
}

static double* stats_part_rows(mdr_ctx* c, int m, int row) {
  return c->d_xstat + ((size_t)x_rank(c) * m + row) * kTickRow;
}

static int stats_rows_combine(mdr_ctx* c, int m, bool closed, double* rows, hipStream_t st) {
  if (closed)
    hipLaunchKernelGGL(k_stats_rows_combine<true>, dim3(m), dim3(64), 0, st, c->kp, c->d_xstat.get(), x_world(c),
                       x_rank(c), m, (const TickArgs*)c->d_ticks.get(), rows);
  else
    hipLaunchKernelGGL(k_stats_rows_combine<false>, dim3(m), dim3(64), 0, st, c->kp, c->d_xstat.get(), x_world(c),
                       x_rank(c), m, (const TickArgs*)nullptr, rows);
  LAUNCH_CHECK("k_stats_rows_combine");
  return MDR_OK;
}

// ONE in-place double sum-allreduce of the call's world x m x 16 slab (every element has exactly one
// non-zero contributor: exact in any order), then the rank-order combine
static int stats_rows_exchange(mdr_ctx* c, int m, bool closed, double* rows, hipStream_t st) {
  if (int rc = comm_allreduce(c, c->d_xstat.get(), (size_t)x_world(c) * m * kTickRow, 1, st)) return rc;
  return stats_rows_combine(c, m, closed, rows, st);
}

int mdr_stats_exchange_ranks(mdr_ctx* c, int world, int rank) {
  if (!c) return fail(MDR_EARG, "mdr_stats_exchange_ranks: null ctx");
  if (world < 1) return fail(MDR_EARG, "mdr_stats_exchange_ranks: world < 1");
  if (rank < 0 || rank >= world) return fail(MDR_EARG, "mdr_stats_exchange_ranks: rank outside [0, world)");
  if (has_comm(c)) {
    if (world != c->world || rank != c->rank)
      return fail(MDR_ESTATE, "mdr_stats_exchange_ranks: the context's communicator has another world / rank");
    return MDR_OK;
  }
  if (world != c->x_world || rank != c->x_rank) {
    HIP_TRY(hipDeviceSynchronize());  // (another layout: no queued combine may still use the slab)
    c->d_xstat.reset();
    c->x_world = world;
    c->x_rank = rank;
  }
  return MDR_OK;
}

// the checks the three slab entry points share, in the order a call with several faults reports them
static int check_stats_exchange(mdr_ctx* c, int m, const char* who) {
  if (!c) return fail(MDR_EARG, std::string(who) + ": null ctx");
  if (m < 1) return fail(MDR_EARG, std::string(who) + ": m < 1");
  if (int rc_ = cluster_ready(c, std::string(who))) return rc_;
  if (!ctx_sharded(c))
    return fail(MDR_ESTATE, std::string(who) + ": neither a communicator nor a shard (single shard: mdr_tick_stats)");
  return MDR_OK;
}

int mdr_stats_exchange_buffer(mdr_ctx* c, int m, double** dev_ptr, int64_t* count) {
  const char* const who = "mdr_stats_exchange_buffer";
  if (!dev_ptr) return fail(MDR_EARG, std::string(who) + ": null dev_ptr");
  if (!count) return fail(MDR_EARG, std::string(who) + ": null count");
  if (int rc = check_stats_exchange(c, m, who)) return rc;
  if (int rc = stats_exchange_reserve(c, m, who)) return rc;
  *dev_ptr = c->d_xstat.get();
  *count = (int64_t)x_world(c) * m * kTickRow;
  return MDR_OK;
}

int mdr_tick_stats_sharded(mdr_ctx* c, const double* reward, const double* p_dev, double p_host, int m, int row,
                           void* stream) {
  const char* const who = "mdr_tick_stats_sharded";
  if (m >= 1 && (row < 0 || row >= m)) return fail(MDR_EARG, std::string(who) + ": row outside [0, m)");
  if (int rc = check_stats_exchange(c, m, who)) return rc;
  if (int rc = stats_exchange_reserve(c, m, who)) return rc;
  if (int rc = tick_scratch(c)) return rc;
  return launch_tick_stats(c, reward, p_dev, p_host, stats_part_rows(c, m, row), S(stream));
}

static int stats_rows_finish(mdr_ctx* c, int m, double* stats, int64_t stats_rows, int64_t stats_row0, void* stream,
                             bool exchange, const char* who) {
  if (int rc = check_stats_rows(who, m, stats_rows, stats_row0)) return rc;
  if (!stats) return fail(MDR_EARG, std::string(who) + ": null stats");
  if (int rc = check_stats_exchange(c, m, who)) return rc;
  if (exchange && !has_comm(c))
    return fail(MDR_ESTATE, std::string(who) + ": no communicator (mdr_rccl_init / mdr_comm_host)");
  if (int rc = stats_exchange_reserve(c, m, who)) return rc;
  double* const rows = stats + (size_t)stats_row0 * kTickRow;
  return exchange ? stats_rows_exchange(c, m, false, rows, S(stream)) : stats_rows_combine(c, m, false, rows, S(stream));
}

int mdr_stats_rows_combine(mdr_ctx* c, int m, double* stats, int64_t stats_rows, int64_t stats_row0, void* stream) {
  return stats_rows_finish(c, m, stats, stats_rows, stats_row0, stream, false, "mdr_stats_rows_combine");
}

int mdr_stats_rows_exchange(mdr_ctx* c, int m, double* stats, int64_t stats_rows, int64_t stats_row0, void* stream) {
  return stats_rows_finish(c, m, stats, stats_rows, stats_row0, stream, true, "mdr_stats_rows_exchange");
}

// ---- replay snapshots (mdr.h mdr_snap): argument checks and the k_snap launch
static int check_snap_struct(const mdr_snap* sn, const char* who) {
  if (sn->struct_bytes != (int32_t)sizeof(mdr_snap))
    return fail(MDR_EARG, std::string(who) + ": mdr_snap.struct_bytes is not sizeof(mdr_snap)");
  return MDR_OK;
}

static int check_snap_slabs(mdr_ctx* c, const mdr_snap* sn, int row0, int nrows, const char* who);

// rows [row0, row0 + nrows) of the caller's slabs can take this context's houses
static int check_snap(mdr_ctx* c, const mdr_snap* sn, int row0, int nrows, const char* who) {
  if (has_comm(c) || c->world > 1)
    return fail(MDR_ESTATE, std::string(who) + ": snapshots are single-shard (a neighbour's rows live on another shard)");
  return check_snap_slabs(c, sn, row0, nrows, who);
}

static int check_snap_slabs(mdr_ctx* c, const mdr_snap* sn, int row0, int nrows, const char* who) {
  if (!sn->t_air || !sn->t_mass || !sn->hvac || !sn->scalars) return fail(MDR_EARG, std::string(who) + ": null snapshot slab");
  if (sn->row_stride < c->kp.n) return fail(MDR_EARG, std::string(who) + ": mdr_snap.row_stride < n_local");
  if (sn->cap_rows < 0 || row0 < 0 || nrows < 0 || (int64_t)row0 + nrows > sn->cap_rows)
    return fail(MDR_EARG, std::string(who) + ": snapshot rows outside [0, cap_rows)");
  return MDR_OK;
}

static int launch_snap(mdr_ctx* c, const mdr_snap* sn, int row, const double* sc_dev, const double* p_dev,
                       const mdr_obs_scalars& sc, hipStream_t st) {
  const int64_t off = (int64_t)row * sn->row_stride;
  const unsigned grid = std::max(1u, std::min(blocks((c->kp.n + 1) / 2, kSnapBlock), (unsigned)kSnapGrid));
  hipLaunchKernelGGL(k_snap, dim3(grid), dim3(kSnapBlock), 0, st, c->kp, sn->t_air + off, sn->t_mass + off,
                     sn->hvac + off, sn->scalars + 4 * (int64_t)row, p_dev, sc_dev, sc.p, sc.s, sc.solar, sc.t_od);
  LAUNCH_CHECK("k_snap");
  return MDR_OK;
}

int mdr_snapshot(mdr_ctx* c, const mdr_snap* sn, int row, const mdr_obs_scalars* sc, const double* p_dev,
                 void* stream) {
  if (sn)
    if (int rc = check_snap_struct(sn, "mdr_snapshot")) return rc;
  if (!c || !sn || !sc) return fail(MDR_EARG, "mdr_snapshot: null argument");
  if (int rc_ = cluster_ready(c, "mdr_snapshot")) return rc_;
  if (int rc = check_snap(c, sn, row, 1, "mdr_snapshot")) return rc;
  return launch_snap(c, sn, row, nullptr, p_dev, *sc, S(stream));
}

int mdr_obs_gather(mdr_ctx* c, const mdr_obs_spec* sp, const mdr_snap* sn, int rows, const int64_t* idx, int64_t m,
                   float* obs, void* stream) {
  if (sn)
    if (int rc = check_snap_struct(sn, "mdr_obs_gather")) return rc;
  if (!c || !sp || !sn || m < 0 || (m > 0 && (!idx || !obs))) return fail(MDR_EARG, "mdr_obs_gather: bad argument");
  if (int rc_ = cluster_ready(c, "mdr_obs_gather")) return rc_;
  if (int rc = check_obs_spec(sp, "mdr_obs_gather")) return rc;
  if (sp->halo_msg || sp->msg_all) return fail(MDR_EARG, "mdr_obs_gather: single shard only (halo_msg / msg_all set)");
  if (int rc = check_snap(c, sn, 0, rows, "mdr_obs_gather")) return rc;
  if (m == 0) return MDR_OK;
  ObsArgs o = obs_args(c, sp, nullptr);
  const size_t tile = ((size_t)kGatherRows * sp->n_feat + 3) & ~(size_t)3;
  const size_t nmsg = (size_t)(sp->comm_mode == MDR_COMM_RING ? sp->n_comm + 1 : 0) * o.msg_w;
  const size_t bytes = (tile + kGatherRows * (nmsg + kObsConst)) * sizeof(float);
  if (bytes > 64 * 1024) return fail(MDR_EARG, "mdr_obs_gather: obs row too wide for one LDS tile");
  if ((m + kGatherRows - 1) / kGatherRows > 0x7fffffffLL)
    return fail(MDR_EARG, "mdr_obs_gather: m too large for one launch");
  hipLaunchKernelGGL(k_obs_gather, dim3(blocks(m, kGatherRows)), dim3(kGatherRows * kGatherLanes), bytes, S(stream),
                     c->kp, o, sn->t_air, sn->t_mass, sn->hvac, sn->row_stride, sn->scalars, rows, idx, m, obs);
  LAUNCH_CHECK("k_obs_gather");
  return MDR_OK;
}

// ---- the sharded forms (mdr.h mdr_snap_halo): the ring halo of the tick beside its snapshot row
static int check_snap_halo_struct(const mdr_snap_halo* hl, const char* who) {
  if (hl->struct_bytes != (int32_t)sizeof(mdr_snap_halo))
    return fail(MDR_EARG, std::string(who) + ": mdr_snap_halo.struct_bytes is not sizeof(mdr_snap_halo)");
  return MDR_OK;
}

// a shard of a larger cluster (its collectives may be the caller's: no communicator) or a context
// with a communicator (world 1 included: the exchanges to self)
static bool ctx_sharded(const mdr_ctx* c) { return has_comm(c) || c->world > 1 || c->kp.n < c->kp.n_global; }

// rows [row0, row0 + nrows) of the halo slab can take `need` floats each
static int check_snap_halo(const mdr_snap_halo* hl, int64_t need, int row0, int nrows, const char* who) {
  if (!hl->rows) return fail(MDR_EARG, std::string(who) + ": null halo slab");
  if (hl->row_stride < need) return fail(MDR_EARG, std::string(who) + ": mdr_snap_halo.row_stride < (lo + hi) * msg_w");
  if (hl->cap_rows < 0 || row0 < 0 || nrows < 0 || (int64_t)row0 + nrows > hl->cap_rows)
    return fail(MDR_EARG, std::string(who) + ": halo rows outside [0, cap_rows)");
  return MDR_OK;
}

// k_snap_halo: snapshot row `row` and nlo floats at halo_lo, nhi at halo_hi into halo row `row`
static int launch_snap_halo(mdr_ctx* c, const mdr_snap* sn, const mdr_snap_halo* hl, int row, const double* sc_dev,
                            const double* p_dev, const mdr_obs_scalars& sc, const float* halo_lo,
                            const float* halo_hi, int nlo, int nhi, hipStream_t st) {
  const int64_t off = (int64_t)row * sn->row_stride;
  const unsigned grid = std::max(1u, std::min(blocks((c->kp.n + 1) / 2, kSnapBlock), (unsigned)kSnapGrid));
  float* hrow = hl && hl->rows ? hl->rows + (int64_t)row * hl->row_stride : nullptr;
  if (!hrow) nlo = nhi = 0;
  hipLaunchKernelGGL(k_snap_halo, dim3(grid), dim3(kSnapBlock), 0, st, c->kp, sn->t_air + off, sn->t_mass + off,
                     sn->hvac + off, sn->scalars + 4 * (int64_t)row, p_dev, sc_dev, sc.p, sc.s, sc.solar, sc.t_od,
                     halo_lo, halo_hi, nlo, nhi, hrow);
  LAUNCH_CHECK("k_snap_halo");
  return MDR_OK;
}

int mdr_snapshot_sharded(mdr_ctx* c, const mdr_obs_spec* sp, const mdr_snap* sn, const mdr_snap_halo* hl, int row,
                         const mdr_obs_scalars* sc, const double* p_dev, const float* halo_src, void* stream) {
  const char* who = "mdr_snapshot_sharded";
  if (sn)
    if (int rc = check_snap_struct(sn, who)) return rc;
  if (hl)
    if (int rc = check_snap_halo_struct(hl, who)) return rc;
  if (!c || !sp || !sn || !sc) return fail(MDR_EARG, std::string(who) + ": null argument");
  if (int rc_ = cluster_ready(c, std::string(who))) return rc_;
  if (!ctx_sharded(c)) return fail(MDR_ESTATE, std::string(who) + ": not a shard and no communicator (mdr_snapshot)");
  if (int rc = check_obs_spec(sp, who)) return rc;
  const int K = sp->n_comm, M = mdr_msg_width(sp), lo = K / 2, hi = (K + 1) / 2;
  if (K > 0 && sp->comm_mode != MDR_COMM_RING)
    return fail(MDR_EARG, std::string(who) + ": across shards only the 'neighbours' ring obs is supported");
  if (int rc = check_snap_slabs(c, sn, row, 1, who)) return rc;
  if (K > 0) {
    if (!hl || !halo_src) return fail(MDR_EARG, std::string(who) + ": the obs reads a ring halo: halo and halo_src must be given");
    if (int rc = check_snap_halo(hl, (int64_t)(lo + hi) * M, row, 1, who)) return rc;
  }
  return launch_snap_halo(c, sn, K > 0 ? hl : nullptr, row, nullptr, p_dev, *sc, halo_src,
                          halo_src ? halo_src + (size_t)lo * M : nullptr, lo * M, hi * M, S(stream));
}

// the obs of this context read a ring halo of other shards' (or, forced, its own) houses
static bool reads_halo(const mdr_ctx* c, const mdr_obs_spec* sp) {
  return sp->n_comm > 0 && sp->comm_mode == MDR_COMM_RING &&
         (c->world > 1 || c->kp.n < c->kp.n_global || c->force_halo);
}

int mdr_obs_gather_sharded(mdr_ctx* c, const mdr_obs_spec* sp, const mdr_snap* sn, const mdr_snap_halo* hl, int rows,
                           const int64_t* idx, int64_t m, float* obs, void* stream) {
  const char* who = "mdr_obs_gather_sharded";
  if (sn)
    if (int rc = check_snap_struct(sn, who)) return rc;
  if (hl)
    if (int rc = check_snap_halo_struct(hl, who)) return rc;
  if (!c || !sp || !sn || m < 0 || (m > 0 && (!idx || !obs))) return fail(MDR_EARG, std::string(who) + ": bad argument");
  if (int rc_ = cluster_ready(c, std::string(who))) return rc_;
  if (!ctx_sharded(c)) return fail(MDR_ESTATE, std::string(who) + ": not a shard and no communicator (mdr_obs_gather)");
  if (int rc = check_obs_spec(sp, who)) return rc;
  if (sp->halo_msg || sp->msg_all)
    return fail(MDR_EARG, std::string(who) + ": halo_msg / msg_all set (the halo comes from the slab)");
  if (sp->n_comm > 0 && sp->comm_mode != MDR_COMM_RING)
    return fail(MDR_EARG, std::string(who) + ": across shards only the 'neighbours' ring obs is supported");
  if (int rc = check_snap_slabs(c, sn, 0, rows, who)) return rc;
  const bool halo = reads_halo(c, sp);
  const int K = sp->n_comm, lo = K / 2, hi = (K + 1) / 2;
  if (halo) {
    if (!hl) return fail(MDR_EARG, std::string(who) + ": the obs reads a ring halo: halo must be given");
    if (int rc = check_snap_halo(hl, (int64_t)(lo + hi) * mdr_msg_width(sp), 0, rows, who)) return rc;
    if (c->kp.n < (lo > hi ? lo : hi)) return fail(MDR_EARG, std::string(who) + ": shard smaller than the ring half-width");
  }
  if (m == 0) return MDR_OK;
  ObsArgs o = obs_args(c, sp, nullptr);
  const size_t tile = ((size_t)kGatherRows * sp->n_feat + 3) & ~(size_t)3;
  const size_t nmsg = (size_t)(sp->comm_mode == MDR_COMM_RING ? sp->n_comm + 1 : 0) * o.msg_w;
  const size_t bytes = (tile + kGatherRows * (nmsg + kObsConst)) * sizeof(float);
  if (bytes > 64 * 1024) return fail(MDR_EARG, std::string(who) + ": obs row too wide for one LDS tile");
  if ((m + kGatherRows - 1) / kGatherRows > 0x7fffffffLL)
    return fail(MDR_EARG, std::string(who) + ": m too large for one launch");
  if (halo) {
    hipLaunchKernelGGL(k_obs_gather_halo, dim3(blocks(m, kGatherRows)), dim3(kGatherRows * kGatherLanes), bytes,
                       S(stream), c->kp, o, sn->t_air, sn->t_mass, sn->hvac, sn->row_stride, sn->scalars, rows, idx, m,
                       obs, (const float*)hl->rows, hl->row_stride);
    LAUNCH_CHECK("k_obs_gather_halo");
  } else {
    hipLaunchKernelGGL(k_obs_gather, dim3(blocks(m, kGatherRows)), dim3(kGatherRows * kGatherLanes), bytes, S(stream),
                       c->kp, o, sn->t_air, sn->t_mass, sn->hvac, sn->row_stride, sn->scalars, rows, idx, m, obs);
    LAUNCH_CHECK("k_obs_gather");
  }
  return MDR_OK;
}

// ---- the actor rollouts: mdr_actor_rollout[_snap|_stats] on one GPU, mdr_actor_rollout_sharded[...]

// a ring halo is exchanged between the shards.  MDR_FORCE_HALO=1 (test hook): even at world 1 (send/recv to self),
// which must reproduce the local ring wrap-around — the 1-GPU check of the multi-GPU exchange
static bool actor_halo(const mdr_ctx* c, const mdr_obs_spec* sp) {
  return (c->world > 1 || c->force_halo) && sp->n_comm > 0;
}

// The argument checks of the six entry points, in the order a call with several faults reports them
// (the single-GPU and the sharded order differ), before anything is staged or launched.
enum { kActorSharded = 1 };
static int actor_rollout_preamble(mdr_ctx* c, const ActorRolloutArgs& a, int flags, hipStream_t st, const char* who) {
  const bool shd = flags & kActorSharded;
  // (deliberate compatibility: these sharded answers name mdr_actor_rollout_sharded whichever of its three was called)
  const std::string base = shd ? "mdr_actor_rollout_sharded" : who;
  int rc;
  if (shd && a.stats && (rc = check_stats_rows(who, a.n, a.stats_rows, a.stats_row0))) return rc;
  if (a.snap && (rc = check_snap_struct(a.snap, who))) return rc;
  if (shd && a.snap && a.shalo && (rc = check_snap_halo_struct(a.shalo, who))) return rc;
  if (!shd && a.stats && (rc = check_stats_rows(who, a.n, a.stats_rows, a.stats_row0))) return rc;
  const bool ptrs = a.ticks && a.osc && a.sp && a.reward && a.p_dev;
  if (!c || !ptrs || a.n < 1) return fail(MDR_EARG, base + ": bad argument");
  if (int rc_ = cluster_ready(c, base)) return rc_;
  if (shd && !has_comm(c)) return fail(MDR_ESTATE, base + ": no communicator (mdr_rccl_init / mdr_comm_host)");
  const bool halo = shd && actor_halo(c, a.sp);
  if (a.snap && !shd && (rc = check_snap(c, a.snap, a.row0, a.n, who))) return rc;
  if (a.snap && shd) {
    if ((rc = check_snap_slabs(c, a.snap, a.row0, a.n, who))) return rc;
    if (halo && !a.shalo) return fail(MDR_EARG, std::string(who) + ": a ring halo is exchanged: halo must be given");
    const int64_t need = (int64_t)a.sp->n_comm * mdr_msg_width(a.sp);
    if (halo && (rc = check_snap_halo(a.shalo, need, a.row0, a.n, who))) return rc;
  }
  if (!shd && a.stats && (rc = check_tick_stats_ctx(c, who))) return rc;
  if ((rc = check_actor_obs(c, a.sp, base.c_str(), st))) return rc;
  if (win_common(c)) return fail(MDR_EARG, base + ": common penalty modes need the per-step API");
  if (halo && a.sp->comm_mode != MDR_COMM_RING)
    return fail(MDR_EARG, base + ": across shards only the 'neighbours' ring obs is supported");
  if (halo && c->kp.n < (a.sp->n_comm + 1) / 2) return fail(MDR_EARG, base + ": shard smaller than the ring half-width");
  return MDR_OK;
}

// ahead of either sequence: the tick drivers, the per-tick obs scalars [s, solar, t_od, -] next to them, d_act
static int actor_stage(mdr_ctx* c, const ActorRolloutArgs& a, hipStream_t st) {
  int rc = refresh_if_dirty(c, st);
  if (!rc) rc = stage_ticks(c, a.n, a.ticks, st);
  if (!rc) rc = stage_recs(a.osc, a.n, c->d_obs_sc, st);
  if (!rc && !a.action) rc = dev_reserve(c->d_act, c->kp.n, "d_act");
  return rc;
}

// The per-tick pieces the three sequences below share.  sp: the obs spec the actor runs (sharded: halo_msg = recv),
// o: its tick-invariant ObsArgs; the ring halo: lo / hi houses before / after the shard, M floats each,
// mine = [hi first | lo last] of this shard, recv = [lo before | hi after]
struct ActorSeq {
  mdr_ctx* c; const ActorRolloutArgs& a; hipStream_t st;
  const mdr_obs_spec* sp; ObsArgs o;
  int lo = 0, hi = 0, M = 0;
  bool halo = false;
  float *mine = nullptr, *recv = nullptr;
  const double* sc(int t) const { return c->d_obs_sc + 4 * t; }  // tick t's staged obs scalars
  ObsArgs obs(int t) const { ObsArgs ot = o; ot.sc_dev = sc(t); return ot; }
  // tick t's outputs (the context-owned action row without the caller's), its ON counts into `counts`
  ActorOut out(int t, unsigned long long* counts) const {
    return ActorOut{a.act_row(t, c->d_act), a.prob_row(t), nullptr, nullptr, counts, nullptr};
  }
  int actor(int t, const ObsArgs& ot, const ActorOut& out) const {
    return launch_actor(c, sp, ot, a.p_dev, 0, c->d_ticks + t, out, st);
  }
  // the state and scalars tick t's actor reads, into snapshot row row0 + t ...
  int snapshot(int t) const {
    return a.snap ? launch_snap(c, a.snap, a.row0 + t, sc(t), a.p_dev, mdr_obs_scalars{}, st) : MDR_OK;
  }
  // ... and the halo it reads, lo rows at halo_lo and hi at halo_hi (none exchanged: an empty halo row)
  int snapshot(int t, const float* halo_lo, const float* halo_hi) const {
    if (!a.snap) return MDR_OK;
    return launch_snap_halo(c, a.snap, halo ? a.shalo : nullptr, a.row0 + t, sc(t), a.p_dev,
                            mdr_obs_scalars{}, halo_lo, halo_hi, lo * M, hi * M, st);
  }
  // this shard's edge rows into mine; their exchange into recv: rank r-1's last lo houses, then rank r+1's first hi
  int pack(hipStream_t on) const {
    hipLaunchKernelGGL(k_halo_pack, dim3(1), dim3(64), 0, on, c->kp, o, lo, hi, mine);
    LAUNCH_CHECK("k_halo_pack");
    return MDR_OK;
  }
  int exchange(hipStream_t on) const { return comm_halo(c, mine, recv, lo, hi, M, on); }
  // tick t's step of its BUFFER actions, from the context's ring of slabs or from explicit ones
  int step(int t) const {
    return launch_step(c, a.act_row(t, c->d_act), MDR_ACT_BUFFER, TickArgs{}, c->d_ticks + t, a.rew_row(t), 0,
                       MDR_CTRL_NONE, nullptr, a.p_dev, st);
  }
  int step(int t, const unsigned long long* cur, unsigned long long* nxt, unsigned long long* zer) const {
    return launch_step_on(c, a.act_row(t, c->d_act), MDR_ACT_BUFFER, TickArgs{}, c->d_ticks + t, a.rew_row(t), 0,
                          MDR_CTRL_NONE, nullptr, a.p_dev, cur, nxt, zer, 0, st);
  }
  // tick t's stats row — the state after its step, its reward row (read before a stride-0 buffer is
  // overwritten by tick t + 1) and P — behind the step, before tick t + 1's snapshot and actor: into the
  // caller's row stats_row0 + t, or (part, sharded) this rank's partial row of the exchange slab
  int row(int t, bool part = false) const {
    if (!a.stats) return MDR_OK;
    return launch_tick_stats(c, a.rew_row(t), a.p_dev, 0.0, part ? stats_part_rows(c, a.n, t) : a.stats_row(t), st);
  }
};

// The single-GPU sequence.  Kernels only, so a graph may capture it.
static int actor_ticks(mdr_ctx* c, const ActorRolloutArgs& a, hipStream_t st) {
  const ActorSeq s{c, a, st, a.sp, obs_args(c, a.sp, &a.osc[0])};
  if (int rc = zero_slabs(c, st)) return rc;
  c->v.slabs_zeroed();
  for (int t = 0; t < a.n; ++t) {
    // the current slab is zero here: the memset above (t = 0), then the previous two steps
    // (each zeroes the slab two ahead and a BUFFER step writes no lookahead)
    if (int rc = s.snapshot(t)) return rc;
    if (int rc = s.actor(t, s.obs(t), s.out(t, slab_at(c, c->v.ring())))) return rc;
    if (int rc = s.step(t)) return rc;
    if (int rc = s.row(t)) return rc;
  }
  return MDR_OK;
}

// The sharded sequence with the halo in the counts (MDR_OPT_HALO_IN_COUNTS): ONE collective per
// tick, the count slab and every rank's post-step edge rows of tick t (the halo of tick t + 1) in one
// integer sum-allreduce (k_halo_step_pack); tick 0's halo (of the current state) is exchanged once
// before the loop.  Tick t counts into slot t % 3 of d_c5, the step kernel's own ring of three.
static int actor_ticks_halo_in_counts(const ActorSeq& s) {
  mdr_ctx* const c = s.c;
  const int lo = s.lo, hi = s.hi, M = s.M, W = lo + hi;
  const size_t rows_words = ((size_t)c->world * W * M + 1) / 2;  // floats, two per u64 word
  const size_t words = c->slab_len + rows_words;
  if (3 * words > c->d_c5.capacity()) {
    HIP_TRY(hipStreamSynchronize(s.st));
    if (int rc = dev_reserve(c->d_c5, 3 * words, "d_c5")) return rc;
  }
  auto buf = [&](int t) { return c->d_c5 + (size_t)(t % 3) * words; };
  auto rows = [&](int t) { return reinterpret_cast<float*>(buf(t) + c->slab_len); };
  hipLaunchKernelGGL(k_zero_u64, dim3(1), dim3(256), 0, s.st, c->d_c5, (int64_t)(3 * words));
  LAUNCH_CHECK("k_zero_u64");
  if (int rc = s.pack(s.st)) return rc;
  if (int rc = s.exchange(s.st)) return rc;
  const int prev = (c->rank + c->world - 1) % c->world, next = (c->rank + 1) % c->world;
  for (int t = 0; t < s.a.n; ++t) {
    // the halo this tick's actor reads: tick 0's from the exchange above, later ticks' the two parts
    // of tick t - 1's allreduced rows, rank prev's last lo and rank next's first hi (stream-ordered
    // after that allreduce, and before this tick's step and the pack of tick t + 2 that next write
    // buf((t - 1) % 3))
    ObsArgs ot = s.obs(t);
    if (t > 0) {
      ot.halo_msg = rows(t - 1) + (size_t)prev * W * M + (size_t)hi * M;
      ot.halo_next = rows(t - 1) + (size_t)next * W * M;
    }
    const ActorOut out = s.out(t, buf(t));
    if (int rc = s.snapshot(t, ot.halo_msg, t > 0 ? ot.halo_next : ot.halo_msg + (size_t)lo * M)) return rc;
    if (int rc = s.actor(t, ot, out)) return rc;
    hipLaunchKernelGGL(k_halo_step_pack, dim3(1), dim3(256), 0, s.st, c->kp, ot, (const uint8_t*)out.action,
                       (const TickArgs*)(c->d_ticks + t), lo, hi, c->rank, c->world, rows(t));
    LAUNCH_CHECK("k_halo_step_pack");
    if (int rc = comm_allreduce(c, buf(t), words, 0, s.st)) return rc;
    if (int rc = s.step(t, buf(t), buf(t + 1), buf(t + 2))) return rc;
    c->v.step_issued(false, false, /*keep_ring=*/true);  // (d_c5's own ring of 3)
    if (int rc = s.row(t, true)) return rc;
  }
  return MDR_OK;
}

// The sharded serial / overlap sequence (config C5): per tick
//   [ring obs across shards] k_halo_pack -> grouped RCCL send/recv of the edge houses' message
//   features with ranks r-1 / r+1 -> k_actor (obs on chip, actions, ON counts of those actions)
//   -> RCCL sum-allreduce of the count slab -> k_step (BUFFER actions, global P)
// Actions are sampled from Philox keyed by (seed, GLOBAL house id, tick) and the counts are exact
// integers, so the sharded run is bit-identical to the single-shard one.
// overlap (fused actor, >= 4 tiles, a comm stream): per tick the halo is packed and exchanged on the
// comm stream while the interior tiles' actor runs on the compute stream; the first and last
// tile follow once it has landed.  They are the only readers of the halo when lo, hi <= 32 and
// the last tile holds no house whose ring reaches past it: tile ntile-2 reads houses up to
// 32 (ntile-1) + hi - 1, beyond the shard when the last tile is short, n % 32 in 1 .. hi-1
static int actor_ticks_sharded(const ActorSeq& s) {
  mdr_ctx* const c = s.c;
  const hipStream_t st = s.st, cs = c->comm_stream;
  HIP_TRY(hipMemsetAsync(c->d_slab, 0, kSlabs * c->slab_len * sizeof(unsigned long long), st));
  c->v.slabs_zeroed();
  const int64_t rag = c->kp.n % 32;
  const bool overlap = s.halo && c->halo_overlap && cs && actor_fused_ok(c, s.sp) && (c->kp.n + 31) / 32 >= 4 &&
                       s.lo <= 32 && s.hi <= 32 && (rag == 0 || rag >= s.hi);
  for (int t = 0; t < s.a.n; ++t) {
    const ObsArgs ot = s.obs(t);
    ActorOut out = s.out(t, slab_at(c, c->v.ring()));
    if (overlap) {
      HIP_TRY(hipEventRecord(c->ev_pc, st));  // the state after the previous step
      HIP_TRY(hipStreamWaitEvent(cs, c->ev_pc, 0));
      if (int rc = s.pack(cs)) return rc;
      ActorOut in = out;
      in.tiles = 1;  // (issued before the exchange: host collectives block in comm_halo)
      if (int rc = s.actor(t, ot, in)) return rc;
      if (int rc = s.exchange(cs)) return rc;
      HIP_TRY(hipEventRecord(c->ev_ar[0], cs));
      HIP_TRY(hipStreamWaitEvent(st, c->ev_ar[0], 0));
      out.tiles = 2;
      // (recv has landed for the compute stream; the next tick's exchange waits on ev_pc, recorded
      // after the snapshot launch below)
    } else if (s.halo) {
      if (int rc = s.pack(st)) return rc;
      if (int rc = s.exchange(st)) return rc;
    }
    // the pre-step state and the halo in recv, before this tick's step
    if (int rc = s.snapshot(t, s.recv, s.recv ? s.recv + (size_t)s.lo * s.M : nullptr)) return rc;
    if (int rc = s.actor(t, ot, out)) return rc;
    if (int rc = comm_allreduce(c, slab_at(c, c->v.ring()), c->slab_len, 0, st)) return rc;
    if (int rc = s.step(t)) return rc;
    if (int rc = s.row(t, true)) return rc;
  }
  return MDR_OK;
}

static ActorGraphKey actor_graph_key(const mdr_ctx* c, ActorRolloutArgs a) {
  if (!a.snap) a.row0 = 0;
  if (!a.stats) a.stats_row0 = 0;
  return ActorGraphKey{a, a.snap ? *a.snap : mdr_snap{}, a.sp->comm_table, a.sp->halo_msg, c->d_actor.get(),
                       a.sp->n_feat, c->actor_head};
}

// mdr_actor_rollout / _snap / _stats: the single-GPU sequence, replayed as a cached graph (the ring at
// the end of its capture: n steps from slab 0, n % 3) unless the caller declines
static int actor_rollout(mdr_ctx* c, const ActorRolloutArgs& a, int use_graph, void* stream, const char* who) {
  enter_writer(c);
  hipStream_t st = S(stream);
  if (int rc = actor_rollout_preamble(c, a, 0, st, who)) return rc;
  Sequence seq(c->v, Sequence::kRollout);
  if (int rc = actor_stage(c, a, st)) return rc;
  if (a.stats)
    if (int rc = tick_scratch(c)) return rc;  // (before any capture)
  auto launches = [&](hipStream_t ls) { return actor_ticks(c, a, ls); };
  if (!use_graph) return seq.end(launches(st));
  return seq.end(replay_graph(c, c->actor_graphs, 1, actor_graph_key(c, a), launches, st));
}

// mdr_actor_rollout_sharded / _snap / _stats.  With a snapshot one k_snap_halo per tick records the
// state, scalars and halo the tick's actor reads; with stats rows each tick leaves this rank's partial
// row and one exchange + combine follows the loop.
static int actor_rollout_sharded(mdr_ctx* c, const ActorRolloutArgs& a, void* stream, const char* who) {
  enter_writer(c);
  hipStream_t st = S(stream);
  if (int rc = actor_rollout_preamble(c, a, kActorSharded, st, who)) return rc;
  if (a.stats) {  // the exchange slab and k_tick_stats' partials, outside the launch sequence
    if (int rc = stats_exchange_reserve(c, a.n, who)) return rc;
    if (int rc = tick_scratch(c)) return rc;
  }
  Sequence seq(c->v, Sequence::kRollout);
  if (int rc = actor_stage(c, a, st)) return rc;
  const int K = a.sp->n_comm, M = mdr_msg_width(a.sp), lo = K / 2, hi = (K + 1) / 2;
  const bool halo = actor_halo(c, a.sp);
  const size_t hrows = (size_t)2 * (lo + hi) * M;
  if (halo && hrows > c->d_halo.capacity()) {
    HIP_TRY(hipStreamSynchronize(st));
    if (int rc = dev_reserve(c->d_halo, hrows, "d_halo")) return rc;
  }
  float* const recv = c->d_halo ? c->d_halo + (size_t)(lo + hi) * M : nullptr;
  mdr_obs_spec spec = *a.sp;
  spec.halo_msg = halo ? recv : nullptr;
  const ActorSeq s{c, a, st, &spec, obs_args(c, &spec, &a.osc[0]), lo, hi, M, halo, c->d_halo, recv};
  int rc = halo && c->halo_in_counts ? actor_ticks_halo_in_counts(s) : actor_ticks_sharded(s);
  if (!rc && a.stats) rc = stats_rows_exchange(c, a.n, false, a.stats_row(0), st);
  return seq.end(rc);
}

int mdr_actor_rollout(mdr_ctx* c, int n, const mdr_tick* ticks, const mdr_obs_scalars* osc, const mdr_obs_spec* sp,
                      uint8_t* action, int64_t act_stride, float* prob, int64_t prob_stride, double* reward,
                      int64_t rew_stride, double* p_dev, int use_graph, void* stream) {
  const ActorRolloutArgs a{n, ticks, osc, sp, action, act_stride, prob, prob_stride, reward, rew_stride, p_dev};
  return actor_rollout(c, a, use_graph, stream, "mdr_actor_rollout");
}

int mdr_actor_rollout_snap(mdr_ctx* c, int n, const mdr_tick* ticks, const mdr_obs_scalars* osc, const mdr_obs_spec* sp,
                           uint8_t* action, int64_t act_stride, float* prob, int64_t prob_stride, double* reward,
                           int64_t rew_stride, double* p_dev, int use_graph, const mdr_snap* snap, int row0,
                           void* stream) {
  const ActorRolloutArgs a{n, ticks, osc, sp, action, act_stride, prob, prob_stride, reward, rew_stride, p_dev,
                           snap, nullptr, row0};
  return actor_rollout(c, a, use_graph, stream, "mdr_actor_rollout_snap");
}

int mdr_actor_rollout_stats(mdr_ctx* c, int n, const mdr_tick* ticks, const mdr_obs_scalars* osc,
                            const mdr_obs_spec* sp, uint8_t* action, int64_t act_stride, float* prob,
                            int64_t prob_stride, double* reward, int64_t rew_stride, double* p_dev, int use_graph,
                            const mdr_snap* snap, int row0, double* stats, int64_t stats_rows, int64_t stats_row0,
                            void* stream) {
  const ActorRolloutArgs a{n, ticks, osc, sp, action, act_stride, prob, prob_stride, reward, rew_stride, p_dev,
                           snap, nullptr, row0, stats, stats_rows, stats_row0};
  return actor_rollout(c, a, use_graph, stream,
                       stats ? "mdr_actor_rollout_stats" : snap ? "mdr_actor_rollout_snap" : "mdr_actor_rollout");
}

int mdr_actor_rollout_sharded(mdr_ctx* c, int n, const mdr_tick* ticks, const mdr_obs_scalars* osc,
                              const mdr_obs_spec* sp, uint8_t* action, int64_t act_stride, float* prob,
                              int64_t prob_stride, double* reward, int64_t rew_stride, double* p_dev, void* stream) {
  const ActorRolloutArgs a{n, ticks, osc, sp, action, act_stride, prob, prob_stride, reward, rew_stride, p_dev};
  return actor_rollout_sharded(c, a, stream, "mdr_actor_rollout_sharded");
}

int mdr_actor_rollout_sharded_snap(mdr_ctx* c, int n, const mdr_tick* ticks, const mdr_obs_scalars* osc,
                                   const mdr_obs_spec* sp, uint8_t* action, int64_t act_stride, float* prob,
                                   int64_t prob_stride, double* reward, int64_t rew_stride, double* p_dev,
                                   const mdr_snap* snap, const mdr_snap_halo* halo, int row0, void* stream) {
  const ActorRolloutArgs a{n, ticks, osc, sp, action, act_stride, prob, prob_stride, reward, rew_stride, p_dev,
                           snap, halo, row0};
  return actor_rollout_sharded(c, a, stream, snap ? "mdr_actor_rollout_sharded_snap" : "mdr_actor_rollout_sharded");
}

int mdr_actor_rollout_sharded_stats(mdr_ctx* c, int n, const mdr_tick* ticks, const mdr_obs_scalars* osc,
                                    const mdr_obs_spec* sp, uint8_t* action, int64_t act_stride, float* prob,
                                    int64_t prob_stride, double* reward, int64_t rew_stride, double* p_dev,
                                    const mdr_snap* snap, const mdr_snap_halo* halo, int row0, double* stats,
                                    int64_t stats_rows, int64_t stats_row0, void* stream) {
  const ActorRolloutArgs a{n, ticks, osc, sp, action, act_stride, prob, prob_stride, reward, rew_stride, p_dev,
                           snap, halo, row0, stats, stats_rows, stats_row0};
  return actor_rollout_sharded(c, a, stream, stats  ? "mdr_actor_rollout_sharded_stats"
                                             : snap ? "mdr_actor_rollout_sharded_snap" : "mdr_actor_rollout_sharded");
}

}  // extern "C"

// ------------------------------------------------------------------------ interpolation (a10)
extern "C" {

int mdr_interp_load(mdr_ctx* c, const mdr_interp_spec* sp) {
  if (!c || !sp || !sp->grid || !sp->values) return fail(MDR_EARG, "mdr_interp_load: null argument");
  InterpArgs a{};
  int64_t ng = 0, total = 1;
  for (int k = 0; k < kInterpAxes; ++k) {
    const bool linear = !(k < 4 || k == 7);
    if (sp->len[k] < (linear ? 2 : 1) || sp->len[k] > (1 << 16))
      return fail(MDR_EARG, "mdr_interp_load: axis length out of range");
    a.len[k] = sp->len[k];
    a.off[k] = (int)ng;
    double lo = sp->grid[ng], hi = sp->grid[ng];
    for (int i = 0; i < sp->len[k]; ++i) {
      const double g = sp->grid[ng + i];
      if (linear && i > 0 && !(g > sp->grid[ng + i - 1]))
        return fail(MDR_EARG, "mdr_interp_load: a linear axis is not strictly ascending");
      lo = g < lo ? g : lo;
      hi = g > hi ? g : hi;
    }
    a.lo[k] = lo;
    a.hi[k] = hi;
    ng += sp->len[k];
  }
  for (int k = kInterpAxes - 1; k >= 0; --k) {
    a.stride[k] = total;
    total *= sp->len[k];
  }
  const int lin[kInterpLinear] = {4, 5, 6, 8, 9};
  for (int q = 0; q < kInterpLinear; ++q) a.lstride[q] = a.stride[lin[q]];
  a.cfg[0] = sp->cfg_ua; a.cfg[1] = sp->cfg_cm; a.cfg[2] = sp->cfg_ca; a.cfg[3] = sp->cfg_hm;
  const size_t bytes = (size_t)(ng + total + MDR_MAX_CAP) * sizeof(double);
  HIP_TRY(hipSetDevice(c->cfg.device));
  HIP_TRY(hipDeviceSynchronize());  // a previous table may still be read by queued launches
  c->interp_ready = false;          // (c->interp views the old table until the copies below succeed)
  if (c->d_interp.reserve(bytes / sizeof(double))) return fail(MDR_ENOMEM, "mdr_interp_load: table");
  HIP_TRY(hipMemcpy(c->d_interp, sp->grid, ng * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->d_interp + ng, sp->values, total * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->d_interp + ng + total, c->cfg.cap_table, MDR_MAX_CAP * sizeof(double),
                    hipMemcpyHostToDevice));
  a.grid = c->d_interp;
  a.table = c->d_interp + ng;
  a.cap = c->d_interp + ng + total;
  c->interp = a;
  c->interp_ready = true;
  return MDR_OK;
}

int mdr_interp_values(mdr_ctx* c, const int64_t* ids, int n, double od, double hour, double date, double* vals,
                      void* stream) {
  if (!c || n < 0 || (n > 0 && (!ids || !vals))) return fail(MDR_EARG, "mdr_interp_values: bad argument");
  if (!c->bound) return fail(MDR_ESTATE, "mdr_interp_values: context not bound");
  if (!c->interp_ready) return fail(MDR_ESTATE, "mdr_interp_values: no table (mdr_interp_load)");
  if (n == 0) return MDR_OK;
  hipLaunchKernelGGL(k_interp_values, dim3(blocks(n, 64)), dim3(64), 0, S(stream), c->kp, c->interp, ids, n,
                     od, hour, date, vals);
  LAUNCH_CHECK("k_interp_values");
  return MDR_OK;
}

int mdr_interp_sum(const double* vals, int n, double factor, double* out, void* stream) {
  if (n < 0 || !out || (n > 0 && !vals)) return fail(MDR_EARG, "mdr_interp_sum: bad argument");
  hipLaunchKernelGGL(k_interp_sum, dim3(1), dim3(64), 0, S(stream), vals, n, factor, out);
  LAUNCH_CHECK("k_interp_sum");
  return MDR_OK;
}

}  // extern "C"
