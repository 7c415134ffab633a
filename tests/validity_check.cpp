// validity_check.cpp — csrc/mdr_validity.h on the CPU (tests/test_validity_cpu.py builds and runs it,
// plain and under AddressSanitizer + UBSan).  Each script raises the transitions in the order an
// entry point of mdr_capi.hip raises them (the matrix) and checks every field the
// section states, the failure paths included: no GPU test may provoke those.
#include <cstdio>

#include "mdr_validity.h"

namespace {

using mdr::EarlyCount;
using mdr::Sequence;
using mdr::SlotsGuard;
using mdr::Validity;

int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                            \
    }                                                                        \
  } while (0)

// ---- the entry points, as sequences of transitions (success paths unless rc is given)
void enter_writer(Validity& v) {
  v.drop_early_count();
  v.state_may_change();
}
void bind(Validity& v) {
  enter_writer(v);
  v.state_replaced();
}
void params_changed(Validity& v) {
  enter_writer(v);
  v.params_replaced();
}
void refresh_if_dirty(Validity& v) {
  if (v.coef_dirty()) v.coef_refreshed();
}
void wslab_clean(Validity& v) {
  if (v.slots_dirty()) v.slots_cleaned();
}
int power_counts(Validity& v, int rc = 0) {
  enter_writer(v);
  Sequence seq(v);
  if (rc) return rc;
  v.counts_produced();
  return seq.ok();
}
int zeroings = 0;  // k_zero_u64 launches over g_hist
void hist_produce(Validity& v) {
  if (v.hist_add()) ++zeroings;
}
void gq_keys(Validity& v, bool slab, bool local_map = true) {
  hist_produce(v);
  if (v.map_stale() && local_map) v.maps_fitted();
  v.keys_from_kernel(512, slab);
}
// mdr_step: epi = the keys come from the step's epilogue (else k_gq_keys behind the step)
int step(Validity& v, bool lookahead, bool keys, bool epi = true, int rc = 0) {
  enter_writer(v);
  if (!v.counts_ready()) return -3;
  Sequence seq(v);
  refresh_if_dirty(v);
  if (rc) return rc;  // (a launch failed)
  if (keys && epi) {
    hist_produce(v);
    v.keys_from_epilogue(40);
  } else if (keys) {
    gq_keys(v, !lookahead);
  }
  v.step_issued(lookahead, keys);
  return seq.ok();
}
// mdr_ctrl_greedy, histogram form: returns whether it used keys already there
bool ctrl_greedy(Validity& v, bool* zeroed_slab = nullptr) {
  const bool ready = v.take_keys();
  enter_writer(v);
  Sequence seq(v);
  if (!ready) gq_keys(v, true);
  else if (!v.slab_zeroed() && zeroed_slab) *zeroed_slab = true;
  v.hist_consumed();
  v.counts_produced();
  seq.ok();
  return ready;
}
int rollout(Validity& v, const EarlyCount& like, int rc = 0) {  // mdr_rollout, the direct window sequence
  v.state_may_change();
  const EarlyCount& b = v.early();
  const bool counted = b.on && b.n == like.n && b.mode == like.mode && b.tick0 == like.tick0;
  if (counted) v.early_consumed();
  else v.drop_early_count();
  Sequence seq(v, Sequence::kRollout);
  refresh_if_dirty(v);
  wslab_clean(v);
  SlotsGuard slots(v);
  if (rc) return rc;
  return seq.end(slots.done());
}
int rollout_begin(Validity& v, const EarlyCount& e, int rc = 0) {
  v.state_may_change();
  v.drop_early_count();
  Sequence seq(v);
  refresh_if_dirty(v);
  wslab_clean(v);
  SlotsGuard slots(v);
  if (rc) return rc;
  slots.done();
  v.early_counted(e);
  return seq.ok();
}
// mdr_greedy_rollout, the fused tick: returns whether the producer had to run first
bool fused_rollout(Validity& v, int n, int* first_parity) {
  const bool ready = v.take_fused();
  enter_writer(v);
  Sequence seq(v, Sequence::kRollout);
  refresh_if_dirty(v);
  int par = v.fused_parity();
  *first_parity = par;
  if (!ready) {
    if (v.map_stale()) v.maps_fitted();
    v.fused_keys_from_kernel(3);
  }
  for (int t = 0; t < n; ++t) {
    v.fused_step_issued(40);
    par = 1 - par;
  }
  v.fused_produced(par);
  seq.ok();
  return !ready;
}

// ---- the scripts
void test_fresh() {
  Validity v;
  CHECK(v.ring() == 0 && !v.counts_ready() && !v.keys_ready() && !v.hist_dirty() && !v.slab_zeroed());
  CHECK(v.map_stale() && v.coef_dirty() && v.slots_dirty() && !v.fused_ready() && !v.early().on);
  CHECK(!v.budget_jumps(1e30, 0.0));  // a NaN history never jumps
}

void test_bind_counts_steps() {
  Validity v;
  bind(v);
  CHECK(!v.counts_ready() && v.coef_dirty() && v.map_stale());
  CHECK(step(v, false, false) == -3);  // no counts: refused before anything moves
  CHECK(v.coef_dirty() && v.ring() == 0);
  CHECK(power_counts(v) == 0 && v.counts_ready() && v.ring() == 0);
  CHECK(step(v, true, false) == 0);  // with a lookahead
  CHECK(v.ring() == 1 && v.counts_ready() && !v.keys_ready() && !v.coef_dirty());
  CHECK(step(v, false, false) == 0);  // without
  CHECK(v.ring() == 2 && !v.counts_ready());
  CHECK(power_counts(v) == 0 && step(v, false, false) == 0 && v.ring() == 0);  // the ring of 3
}

void test_keys_take_consume() {
  Validity v;
  bind(v);
  power_counts(v);
  zeroings = 0;
  CHECK(step(v, false, true) == 0);  // keys by the epilogue
  CHECK(v.keys_ready() && v.hist_dirty() && v.slab_zeroed() && v.nparts() == 40 && zeroings == 0);
  CHECK(ctrl_greedy(v));  // took them
  CHECK(!v.keys_ready() && !v.hist_dirty() && v.counts_ready() && zeroings == 0);
  CHECK(!ctrl_greedy(v));  // a second call has none to take: k_gq_keys, and it fits the maps
  CHECK(!v.map_stale() && v.nparts() == 512 && v.slab_zeroed() && !v.hist_dirty());
  // keys beside a lookahead (k_gq_keys behind the step, no slab): the decisions' slab holds counts
  CHECK(step(v, true, true, false) == 0 && v.keys_ready() && !v.slab_zeroed() && v.counts_ready());
  bool zeroed = false;
  CHECK(ctrl_greedy(v, &zeroed) && zeroed);
}

void test_two_producers() {
  Validity v;
  bind(v);
  power_counts(v);
  zeroings = 0;
  CHECK(step(v, true, true) == 0 && zeroings == 0);  // producer 1
  CHECK(step(v, true, true) == 0 && zeroings == 1);  // producer 2, no consumer between: zero first
  CHECK(ctrl_greedy(v) && !v.hist_dirty());
  CHECK(step(v, false, true) == 0 && zeroings == 1);  // consumed: nothing to zero
}

void test_params_between_producer_and_take() {
  Validity v;
  bind(v);
  ctrl_greedy(v);  // (the first decision's k_gq_keys fits the maps; an epilogue's keys never do)
  CHECK(!v.map_stale());
  v.budget_decided(1.0), v.budget_decided(2.0);
  CHECK(v.budget_jumps(100.0, 1.0) && !v.budget_jumps(3.0, 1.0));
  step(v, true, true);
  CHECK(v.keys_ready() && v.counts_ready());
  params_changed(v);
  CHECK(!v.keys_ready() && v.map_stale() && v.coef_dirty() && v.hist_dirty());
  CHECK(v.counts_ready());                // mdr_params_changed leaves the counts
  CHECK(!v.budget_jumps(100.0, 1.0));     // the history is NaN again
  zeroings = 0;
  CHECK(!ctrl_greedy(v) && zeroings == 1 && !v.map_stale());  // new keys over a zeroed histogram, maps re-fitted
  // a sharded producer (local_map = false) must not fit the maps
  params_changed(v);
  gq_keys(v, false, false);
  CHECK(v.map_stale());
}

void test_scratch_regrown() {
  Validity v;
  bind(v);
  power_counts(v);
  step(v, false, true);
  CHECK(v.keys_ready() && v.hist_dirty());
  v.scratch_regrown();
  CHECK(!v.keys_ready() && !v.hist_dirty() && !v.fused_ready());
  v.fused_produced(1);
  v.fused_scratch_regrown();
  CHECK(!v.fused_ready() && v.fused_parity() == 0);
}

void test_early_count() {
  const EarlyCount e{true, 9, 1, 100, nullptr, 0, false};
  EarlyCount other = e;
  other.n = 8;
  {  // a matching rollout consumes it: the slots stay clean
    Validity v;
    bind(v);
    CHECK(rollout_begin(v, e) == 0 && v.early().on && v.early().n == 9 && !v.slots_dirty() && !v.coef_dirty());
    CHECK(rollout(v, e) == 0 && !v.early().on && !v.slots_dirty() && !v.counts_ready());
  }
  {  // a mismatching one drops it: dirty until wslab_clean, clean again behind the sequence
    Validity v;
    bind(v);
    rollout_begin(v, e);
    v.state_may_change();
    v.drop_early_count();
    CHECK(!v.early().on && v.slots_dirty());
    CHECK(rollout(v, other) == 0 && !v.slots_dirty());
  }
  {  // an unrelated entry point
    Validity v;
    bind(v);
    rollout_begin(v, e);
    CHECK(power_counts(v) == 0 && !v.early().on && v.slots_dirty() && v.counts_ready());
  }
  {  // a second begin drops the first; nothing outstanding: the slots stay as they are
    Validity v;
    bind(v);
    rollout_begin(v, e);
    CHECK(rollout_begin(v, other) == 0 && v.early().on && v.early().n == 8 && !v.slots_dirty());
    rollout(v, other);
    v.drop_early_count();
    CHECK(!v.slots_dirty());
  }
  {  // the sites kept for compatibility (mdr_set_option, ...): an early count dropped, and the keys
    Validity v;
    bind(v);
    power_counts(v);
    step(v, true, true);
    rollout_begin(v, e);
    CHECK(!v.keys_ready());  // (mdr_rollout_begin's preamble already says the state may change)
    enter_writer(v);
    CHECK(!v.early().on && v.slots_dirty() && v.counts_ready());
    v.map_form_switched();
    CHECK(v.map_stale());
  }
}

void test_slots_guard() {
  Validity v;
  v.slots_cleaned();
  {
    SlotsGuard g(v);
    CHECK(v.slots_dirty());
    CHECK(g.done() == 0);
  }
  CHECK(!v.slots_dirty());
  {
    SlotsGuard g(v);  // an early return
  }
  CHECK(v.slots_dirty());
}

void test_failures() {
  const EarlyCount e{true, 9, 1, 100, nullptr, 0, false};
  {  // a rollout fails behind its first launch: nothing derived is vouched for
    Validity v;
    bind(v);
    power_counts(v);
    step(v, true, true);
    v.fused_produced(1);
    v.counts_produced();
    CHECK(rollout(v, e, -2) == -2);
    CHECK(!v.counts_ready() && !v.keys_ready() && !v.fused_ready() && v.slots_dirty() && !v.early().on);
    CHECK(!v.coef_dirty());  // (k_refresh was issued before the failure: cleared behind its own launch)
  }
  {  // the rollout-exit guard on success: the counts go, the rest stays
    Validity v;
    bind(v);
    power_counts(v);
    CHECK(rollout(v, e) == 0 && !v.counts_ready() && !v.slots_dirty());
  }
  {  // a failing early count leaves none outstanding and the slots dirty
    Validity v;
    bind(v);
    CHECK(rollout_begin(v, e, -2) == -2 && !v.early().on && v.slots_dirty());
  }
  {  // a failing step: the lookahead's counts of the tick before are not vouched for either
    Validity v;
    bind(v);
    power_counts(v);
    CHECK(step(v, true, true, true, -2) == -2 && !v.counts_ready() && !v.keys_ready() && v.ring() == 0);
  }
  {  // a failing call never clears coef_dirty / map_stale that its launches did not reach
    Validity v;
    bind(v);
    {
      Sequence seq(v);
    }
    CHECK(v.coef_dirty() && v.map_stale());
    CHECK(power_counts(v, -2) == -2 && !v.counts_ready());
  }
  {  // end(rc)
    Validity v;
    v.counts_produced();
    {
      Sequence seq(v);
      CHECK(seq.end(0) == 0);
    }
    CHECK(v.counts_ready());
    {
      Sequence seq(v);
      CHECK(seq.end(-5) == -5);
    }
    CHECK(!v.counts_ready());
  }
}

void test_fused() {
  Validity v;
  bind(v);
  int p0 = -1;
  CHECK(fused_rollout(v, 3, &p0) && p0 == 0);  // nothing ready: the producer runs, parity 0 first
  CHECK(v.fused_ready() && v.fused_parity() == 1 && v.ring() == 0 && !v.counts_ready() && !v.keys_ready());
  CHECK(!v.map_stale() && v.nparts() == 40);
  CHECK(!fused_rollout(v, 2, &p0) && p0 == 1);  // ready: continues from the parity the last step wrote
  CHECK(v.fused_ready() && v.fused_parity() == 1 && v.ring() == 2);
  CHECK(!fused_rollout(v, 1, &p0) && p0 == 1 && v.fused_parity() == 0);
  // a per-tick greedy call in between: the fused products are of an older state afterwards
  ctrl_greedy(v);
  CHECK(!v.fused_ready());
  CHECK(fused_rollout(v, 1, &p0) && p0 == 0);
  // the explicit-slab step (the sharded sequencers) and the slabs' zeroing
  v.counts_produced();
  v.step_issued(true, false, true);
  CHECK(v.ring() == 1 && v.counts_ready() && !v.fused_ready());
  v.slabs_zeroed();
  CHECK(v.ring() == 0 && !v.counts_ready());
  v.graph_replayed(2);
  CHECK(v.ring() == 2);
  v.counts_produced();
  v.counts_lost();
  CHECK(!v.counts_ready());
}

}  // namespace

int main() {
  test_fresh();
  test_bind_counts_steps();
  test_keys_take_consume();
  test_two_producers();
  test_params_between_producer_and_take();
  test_scratch_regrown();
  test_early_count();
  test_slots_guard();
  test_failures();
  test_fused();
  if (failures) {
    std::fprintf(stderr, "validity_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("validity_check: ok\n");
  return 0;
}
