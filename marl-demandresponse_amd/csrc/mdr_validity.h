// mdr_validity.h — what the host believes the context's device buffers currently hold.
// Host-only and free of HIP names, so its rules are checked on the CPU (tests/validity_check.cpp).
// mdr_capi.hip says what happened (a transition); which fields that moves is decided here alone.
#pragma once

#include <cmath>
#include <cstdint>

namespace mdr {

// mdr_rollout_begin: the first window of exactly this rollout is already counted
struct EarlyCount {
  bool on = false;
  int n = 0, mode = 0;
  uint64_t tick0 = 0;
  const uint8_t* action = nullptr;
  int64_t act_stride = 0;
  bool sharded = false;  // counts allreduced over the ranks (for mdr_rollout_sharded)
};

// The first group of windows of the NEXT direct rollout, counted by the last step launch of the
// previous one (its speculative lookahead): mask rows, end words and slot shards are on
// the device for exactly the call {n, mode, tick0} under {window, group}, issued on `stream`.
constexpr int kCarryGroup = 4;  // = kWinGroup
constexpr int kCarrySlots = 8;  // = kWinSlots
struct CarriedCount {
  bool on = false;
  int n = 0, mode = 0;
  uint64_t tick0 = 0;      // the counted call's first tick id
  int window = 0, group = 0;
  int nw = 0;              // windows counted: the call's first min(group, windows)
  int K[kCarryGroup] = {};  // their ticks
  int slot_base = 0;       // window w of the counted call is in slot carry_slot(slot_base, w)
  const void* stream = nullptr;
  int half = 0;            // the half of the group mask rows that holds the counted windows' rows (group_half)
};
// window w of a call whose first window is in slot `base`; the call after one of nw windows starts at
// carry_slot(base, nw): consecutive windows take consecutive slots across the call boundary, so a
// launch's stepped group (<= kCarryGroup) and counted group (<= kCarryGroup) never share a slot
constexpr int carry_slot(int base, int w) { return (base + w) % kCarrySlots; }
// The group mask rows come in two halves: a step launch reads its windows' rows from one and writes the
// counted windows' rows to the other (so a block may count before it steps).  The KA launch of a plain
// call reads the count kernel's rows and writes half 0; a carried call starts from the half its record
// names.  The k-th group launch of a call (from 0) reads half group_half(carried, half_in, k) and writes
// the other; behind a call of L group launches the counted rows are in group_half(carried, half_in, L).
constexpr int group_half(bool carried, int half_in, int k) { return ((carried ? half_in : 0) + k) & 1; }
// the group launches of a call of nw windows in groups of G (a plain call's first window goes to the KA launch)
constexpr int group_launches(bool carried, int nw, int G) { return ((carried ? nw : nw - 1) + G - 1) / G; }

// the last direct grouped rollout that could have speculated (the shape the next one must continue)
struct DirectCall {
  bool on = false;
  int n = 0, mode = 0, window = 0, group = 0;
  uint64_t next_tick = 0;  // its last tick id + 1
  const void* stream = nullptr;
};

struct CarryCounters {
  int64_t speculated = 0, consumed = 0, dropped = 0;
};

class Validity {
 public:
  // ---- queries
  int ring() const { return ring_; }                    // slab of the current tick
  bool counts_ready() const { return counts_ready_; }   // ... holds this tick's cluster-power counts
  bool slab_zeroed() const { return slab_zeroed_; }     // the codes' producer zeroed the decisions' slab
  bool map_stale() const { return map_stale_; }         // state / parameters written since the maps were fitted
  int nparts() const { return nparts_; }                // (min, max) partials of the last key producer
  int fused_parity() const { return fz_par_; }          // the parity the last fused producer wrote
  bool coef_dirty() const { return coef_dirty_; }       // k_refresh must run before the next launch sequence
  bool slots_dirty() const { return slots_dirty_; }     // the window slots' shard part is not known to be zero
  const EarlyCount& early() const { return early_; }
  const CarriedCount& carry() const { return carry_; }
  const CarryCounters& carry_counters() const { return carry_n_; }
  // the carried count is of exactly this call (the options it was planned under still hold)
  bool carry_matches(int n, int mode, uint64_t tick0, int window, int group, const void* stream) const {
    return carry_.on && carry_.n == n && carry_.mode == mode && carry_.tick0 == tick0 && carry_.window == window &&
           carry_.group == group && carry_.stream == stream;
  }
  // this call continues the previous direct call: same shape, the next tick id (so it may speculate)
  bool continues_direct(int n, int mode, uint64_t tick0, int window, int group, const void* stream) const {
    return last_.on && last_.n == n && last_.mode == mode && last_.next_tick == tick0 && last_.window == window &&
           last_.group == group && last_.stream == stream;
  }
  bool keys_ready() const { return keys_ready_; }       // (the checks; the library takes them: take_keys)
  bool hist_dirty() const { return hist_dirty_; }
  bool fused_ready() const { return fz_ready_; }
  // the adaptive band: the change to `budget` departs from the last change by more than `jump`
  // (never while the history is NaN: after the parameters were replaced)
  bool budget_jumps(double budget, double jump) const {
    return s1_ == s1_ && s2_ == s2_ && !(std::fabs((budget - s1_) - (s1_ - s2_)) <= jump);
  }

  // ---- the house state, the parameters
  // mdr_bind / mdr_populate: the arrays or their contents replaced
  void state_replaced() {
    counts_ready_ = false;
    params_replaced();
  }
  // mdr_params_changed (the counts stay: they are of the actions, and the caller vouches for those)
  void params_replaced() {
    drop_carry();  // (the FSM words or the class indices may be new)
    last_.on = false;
    coef_dirty_ = true;
    map_stale_ = true;
    s1_ = s2_ = NAN;
  }
  void coef_refreshed() { coef_dirty_ = false; }
  // an entry point that may write the house state, the count slabs, the mask rows or the window slots
  // is entered.  keep_carry: mdr_rollout / mdr_rollout_begin, which settle the carried count
  // themselves (consume it, or drop it) once their arguments are checked
  void state_may_change(bool keep_carry = false) {
    keys_ready_ = false;
    fz_ready_ = false;
    if (!keep_carry) {
      drop_carry();
      last_.on = false;
    }
  }

  // ---- the count slabs
  // all slabs zeroed: the sequence counts from slab 0
  void slabs_zeroed() {
    ring_ = 0;
    counts_ready_ = false;
  }
  void counts_produced() { counts_ready_ = true; }  // of the current tick, into the current slab
  void counts_lost() { counts_ready_ = false; }     // the slabs overwritten, or a rollout behind them
  // a step was issued: the next slab is current, filled if the step counted a lookahead; the state
  // moved, so only this step's own epilogue vouches for keys.  keep_ring: explicit slabs (launch_step_on)
  void step_issued(bool lookahead, bool keys_epilogue, bool keep_ring = false) {
    if (!keep_ring) ring_ = (ring_ + 1) % 3;
    counts_ready_ = lookahead;
    keys_ready_ = keys_epilogue;
    fz_ready_ = false;
  }
  // the fused tick's step (GQ = 2 epilogue, no lookahead): its products are vouched for by fused_produced
  void fused_step_issued(int nparts) {
    ring_ = (ring_ + 1) % 3;
    counts_ready_ = false;
    keys_ready_ = false;
    nparts_ = nparts;
  }
  // a cached graph replayed: the ring as the captured sequence left it
  void graph_replayed(int ring_at_end) { ring_ = ring_at_end; }

  // ---- greedy keys, histogram, maps
  bool take_keys() {  // were they of the current state?  The caller consumes them
    const bool r = keys_ready_;
    keys_ready_ = false;
    return r;
  }
  void keys_from_kernel(int nparts, bool slab_zeroed) {  // k_gq_keys (slab given: zeroed for the decisions)
    nparts_ = nparts;
    slab_zeroed_ = slab_zeroed;
  }
  void keys_from_epilogue(int nparts) {  // the GQ = 1 step epilogue zeroes its next slab (no lookahead)
    nparts_ = nparts;
    slab_zeroed_ = true;
  }
  bool hist_add() {  // a producer is about to add to g_hist: must it be zeroed first?
    const bool r = hist_dirty_;
    hist_dirty_ = true;
    return r;
  }
  void hist_consumed() { hist_dirty_ = false; }
  void maps_fitted() { map_stale_ = false; }
  void map_form_switched() { map_stale_ = true; }  // MDR_OPT_GQ_FUSED: the other form's map is of an older state
  void budget_decided(double budget) {
    s2_ = s1_;
    s1_ = budget;
  }
  void scratch_regrown() {  // greedy_scratch: new buffers hold nothing
    keys_ready_ = false;
    fz_ready_ = false;
    hist_dirty_ = false;
  }
  // the fused tick
  bool take_fused() {
    const bool r = fz_ready_;
    fz_ready_ = false;
    return r;
  }
  void fused_keys_from_kernel(int nparts) { nparts_ = nparts; }  // k_gq_keys2
  void fused_produced(int parity) {  // the last fused step's epilogue wrote `parity` for the current state
    fz_par_ = parity;
    fz_ready_ = true;
    counts_ready_ = false;
  }
  void fused_scratch_regrown() {
    fz_ready_ = false;
    fz_par_ = 0;
  }

  // ---- window slots, the early count
  void slots_cleaned() { slots_dirty_ = false; }
  void drop_early_count() {  // nobody consumed it: its shards are still in the slot
    if (early_.on) {
      early_.on = false;
      slots_dirty_ = true;
    }
  }
  void early_consumed() { early_.on = false; }  // by the rollout it was counted for
  void early_counted(const EarlyCount& e) {
    early_ = e;
    early_.on = true;
  }

  // ---- the carried count (the next direct rollout's first group)
  void drop_carry() {  // nobody will consume it: its shards are still in the slots
    if (carry_.on) {
      carry_.on = false;
      slots_dirty_ = true;
      carry_n_.dropped += 1;
    }
    carry_.half = 0;  // (a call that starts from no record starts at half 0)
  }
  void carry_consumed() {  // by the rollout it was counted for
    if (carry_.on) carry_n_.consumed += 1;
    carry_.on = false;
    carry_.half = 0;  // (the consumer took it with the slot base before this)
  }
  void carry_counted(const CarriedCount& k) {  // behind the fully issued sequence whose last launch counted it
    carry_ = k;
    carry_.on = true;
    carry_n_.speculated += 1;
  }
  // a direct grouped rollout that may carry was fully issued / another rollout ran instead
  void direct_call_issued(const DirectCall& d) {
    last_ = d;
    last_.on = true;
  }
  void direct_call_forgotten() { last_.on = false; }

  // ---- a sequence failed part-way: nothing derived is vouched for (coef_dirty and map_stale are
  // only ever cleared behind their own launches, so they stay as they are)
  void sequence_failed() {
    counts_ready_ = false;
    keys_ready_ = false;
    fz_ready_ = false;
    slots_dirty_ = true;
    early_.on = false;
    if (carry_.on) carry_n_.dropped += 1;
    carry_.on = false;
    carry_.half = 0;
    last_.on = false;
  }

 private:
  friend class SlotsGuard;
  int ring_ = 0;
  bool counts_ready_ = false;
  bool keys_ready_ = false;
  bool hist_dirty_ = false;
  bool slab_zeroed_ = false;
  bool map_stale_ = true;
  bool fz_ready_ = false;
  int fz_par_ = 0;
  int nparts_ = 0;
  bool coef_dirty_ = true;
  bool slots_dirty_ = true;
  EarlyCount early_{};
  CarriedCount carry_{};
  DirectCall last_{};
  CarryCounters carry_n_{};
  double s1_ = NAN, s2_ = NAN;  // the last two budgets mdr_greedy_rollout decided for
};

// The window slots are dirty until the sequence that counts into them is fully issued: an early
// return leaves them dirty (wslab_clean zeroes them before the next rollout).
class SlotsGuard {
 public:
  explicit SlotsGuard(Validity& v) : v_(v) { v_.slots_dirty_ = true; }
  SlotsGuard(const SlotsGuard&) = delete;
  SlotsGuard& operator=(const SlotsGuard&) = delete;
  int done() {  // (returns 0, the sequencer's MDR_OK)
    v_.slots_dirty_ = false;
    return 0;
  }

 private:
  Validity& v_;
};

// From an entry point's first launch or host-state change to its return.  A return that did not
// pass through ok() / end(0) is a failure: sequence_failed().  kRollout: the call leaves the state
// many ticks on, so no slab holds the next tick's counts, whether it succeeded or not.
class Sequence {
 public:
  enum Kind { kCall, kRollout };
  explicit Sequence(Validity& v, Kind k = kCall) : v_(v), kind_(k) {}
  Sequence(const Sequence&) = delete;
  Sequence& operator=(const Sequence&) = delete;
  ~Sequence() {
    if (!ok_) v_.sequence_failed();
    else if (kind_ == kRollout) v_.counts_lost();
  }
  int ok() { return end(0); }
  int end(int rc) {
    ok_ = rc == 0;
    return rc;
  }

 private:
  Validity& v_;
  Kind kind_;
  bool ok_ = false;
};

}  // namespace mdr
