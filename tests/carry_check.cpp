// carry_check.cpp — the carried count of csrc/mdr_validity.h (CarriedCount) on the CPU
// (tests/test_carry_cpu.py builds and runs it, plain and under AddressSanitizer + UBSan).  The entry
// points are the sequences of transitions mdr_capi.hip raises; every transition that can invalidate a
// count made for the next call must drop it, and the slots must run on across call boundaries.
// rollout() and rollout_begin() below are a MODEL of mdr_rollout and mdr_rollout_begin (as
// validity_check.cpp's scripts are of their entry points): they pin the rules of Validity, not the
// code of mdr_capi.hip, whose own conditions (the source, window_ok, consecutive ids) they leave out.
// The real composition runs in tests/test_rollout_carry_gpu.py, which asserts the same counters.
#include <cstdio>
#include <set>
#include <utility>
#include <vector>

#include "mdr_validity.h"

namespace {

using mdr::CarriedCount;
using mdr::DirectCall;
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

constexpr int kRandom = 1, kAlwaysOn = 2;
int stream_a, stream_b;  // (two stream handles)

struct Ctx {  // what of the context the carry rules read
  Validity v;
  int win = 7, group = 4;
  bool carry = true;
  int cleans = 0;  // wslab_clean's memsets
};

int windows(int n, int win) { return (n + win - 1) / win; }  // WinPlan::count

void enter_writer(Validity& v) {
  v.drop_early_count();
  v.state_may_change();
}

// mdr_rollout_begin: true when a matching carry made it launch nothing
bool rollout_begin(Ctx& c, int n, int mode, uint64_t tick0, const void* st = &stream_a) {
  c.v.state_may_change(true);
  c.v.drop_early_count();
  if (c.carry && c.v.carry_matches(n, mode, tick0, c.win, c.group, st)) return true;
  c.v.drop_carry();
  Sequence seq(c.v);
  if (c.v.slots_dirty()) c.v.slots_cleaned(), ++c.cleans;
  SlotsGuard slots(c.v);
  slots.done();
  mdr::EarlyCount e{};
  e.n = n, e.mode = mode, e.tick0 = tick0;
  c.v.early_counted(e);
  seq.ok();
  return false;
}

struct Ran {
  bool carried, speculated;
  int slot_base;
};

// mdr_rollout, the direct grouped sequence of an eligible source (graph: the staged sequence instead)
Ran rollout(Ctx& c, int n, int mode, uint64_t tick0, bool graph = false, int rc = 0, const void* st = &stream_a) {
  c.v.state_may_change(true);
  const bool may = !graph && c.carry && c.group > 0;
  Ran r{may && c.v.carry_matches(n, mode, tick0, c.win, c.group, st), false, 0};
  if (r.carried) {
    r.slot_base = c.v.carry().slot_base;
    c.v.carry_consumed();
  } else {
    c.v.drop_carry();
  }
  r.speculated = may && c.v.continues_direct(n, mode, tick0, c.win, c.group, st);
  c.v.direct_call_forgotten();
  if (!r.carried && c.v.early().on && c.v.early().n == n && c.v.early().tick0 == tick0) c.v.early_consumed();
  else c.v.drop_early_count();
  Sequence seq(c.v, Sequence::kRollout);
  if (c.v.slots_dirty()) {
    CHECK(!r.carried);  // (a carried call's slots are never cleared under it)
    c.v.slots_cleaned(), ++c.cleans;
  }
  SlotsGuard slots(c.v);
  if (rc) {
    seq.end(rc);
    return r;
  }
  slots.done();
  if (may) {
    const int nw = windows(n, c.win);
    c.v.direct_call_issued(DirectCall{true, n, mode, c.win, c.group, tick0 + (uint64_t)n, st});
    if (r.speculated) {
      CarriedCount k{};
      k.n = n, k.mode = mode, k.tick0 = tick0 + (uint64_t)n, k.window = c.win, k.group = c.group;
      k.nw = c.group < nw ? c.group : nw;
      k.slot_base = mdr::carry_slot(r.slot_base, nw);
      k.stream = st;
      c.v.carry_counted(k);
    }
  }
  seq.ok();
  return r;
}

// a context with a carry outstanding for (40, random, tick 120): three calls
void armed(Ctx& c) {
  for (int i = 0; i < 3; ++i) {
    rollout_begin(c, 40, kRandom, 40u * i);
    rollout(c, 40, kRandom, 40u * i);
  }
  CHECK(c.v.carry().on && c.v.carry().tick0 == 120);
  CHECK(c.v.carry_counters().speculated == 2 && c.v.carry_counters().consumed == 1 &&
        c.v.carry_counters().dropped == 0);
  CHECK(!c.v.slots_dirty());
}

void script_six_calls() {
  Ctx c;
  for (int i = 0; i < 6; ++i) {
    const bool quiet = rollout_begin(c, 40, kRandom, 40u * i);
    const Ran r = rollout(c, 40, kRandom, 40u * i);
    CHECK(quiet == (i >= 2) && r.carried == (i >= 2) && r.speculated == (i >= 1));
  }
  const mdr::CarryCounters& k = c.v.carry_counters();
  CHECK(k.speculated == 5 && k.consumed == 4 && k.dropped == 0 && c.v.carry().on);
  Ctx off;
  off.carry = false;
  for (int i = 0; i < 6; ++i) {
    CHECK(!rollout_begin(off, 40, kRandom, 40u * i));
    const Ran r = rollout(off, 40, kRandom, 40u * i);
    CHECK(!r.carried && !r.speculated);
  }
  CHECK(off.v.carry_counters().speculated == 0 && off.v.carry_counters().consumed == 0 &&
        off.v.carry_counters().dropped == 0);
}

// every transition that can invalidate the carry drops it once and marks the slots dirty (ran: f is
// itself a sequence, which cleared them once before it counted), and the next call does not start
// from it
template <typename F>
void dropped_by(const char* what, F&& f, bool ran = false, bool next_continues = false) {
  Ctx c;
  armed(c);
  CHECK(c.cleans == 1);  // (the new context's)
  f(c);
  if (c.v.carry().on || c.v.carry_counters().dropped != 1 || (ran ? c.cleans != 2 : !c.v.slots_dirty())) {
    std::fprintf(stderr, "carry not dropped by: %s\n", what);
    ++failures;
  }
  rollout_begin(c, 40, kRandom, 120);
  const Ran r = rollout(c, 40, kRandom, 120);
  CHECK(!r.carried && r.speculated == next_continues);
  CHECK(c.v.carry_counters().dropped == 1);
}

void script_drops() {
  dropped_by("state_replaced (mdr_bind, mdr_populate)", [](Ctx& c) { enter_writer(c.v), c.v.state_replaced(); });
  dropped_by("params_replaced (mdr_params_changed)", [](Ctx& c) { enter_writer(c.v), c.v.params_replaced(); });
  dropped_by("params_replaced alone", [](Ctx& c) { c.v.params_replaced(); });
  dropped_by("state_may_change (any other entry point: options, step_tensor, graph and closed-loop rollouts, "
             "returns, stats, sharded, greedy and actor rollouts, mdr_time_step_kernels)",
             [](Ctx& c) { enter_writer(c.v); });
  dropped_by("sequence_failed", [](Ctx& c) { c.v.sequence_failed(); });
  dropped_by("mdr_rollout with a graph", [](Ctx& c) { rollout(c, 40, kRandom, 120, true); }, true);
  dropped_by("another n", [](Ctx& c) { rollout(c, 23, kRandom, 120); }, true);
  dropped_by("another source", [](Ctx& c) { rollout(c, 40, kAlwaysOn, 120); }, true);
  dropped_by("another tick id", [](Ctx& c) { rollout(c, 40, kRandom, 121); }, true);
  dropped_by("another stream", [](Ctx& c) { rollout(c, 40, kRandom, 120, false, 0, &stream_b); }, true);
  dropped_by("mdr_rollout_begin for another call", [](Ctx& c) { rollout_begin(c, 40, kRandom, 200); }, true, true);
  dropped_by("mdr_set_rollout_window", [](Ctx& c) { enter_writer(c.v), c.win = 5; });
  dropped_by("MDR_OPT_WINDOW_GROUP", [](Ctx& c) { enter_writer(c.v), c.group = 2; });
  dropped_by("MDR_OPT_ROLLOUT_CARRY 0 without the option's entry", [](Ctx& c) {
    c.carry = false;
    rollout(c, 40, kRandom, 120);
    c.carry = true;
  }, true);
  // a carried call that fails part-way consumed the count: the slots are dirty, nothing is outstanding
  Ctx c;
  armed(c);
  const Ran r = rollout(c, 40, kRandom, 120, false, -2);
  CHECK(r.carried && !c.v.carry().on && c.v.slots_dirty() && c.v.carry_counters().dropped == 0);
  const Ran next = rollout(c, 40, kRandom, 120);
  CHECK(!next.carried && !next.speculated && c.cleans == 2);
}

// consecutive windows take consecutive slots across call boundaries: in every launch the stepped
// group's slots and the counted group's are distinct, and a carried call finds its windows where the
// previous call's last launch counted them
void script_slots() {
  const int nws[4] = {1, 3, 4, 6};
  for (int nw : nws)
    for (int group = 1; group <= mdr::kCarryGroup; ++group) {
      Ctx c;
      c.group = group;
      const int n = nw * c.win;
      int expect_base = 0;
      for (int call = 0; call < 20; ++call) {
        rollout_begin(c, n, kRandom, (uint64_t)n * call);
        const Ran r = rollout(c, n, kRandom, (uint64_t)n * call);
        CHECK(r.carried == (call >= 2));
        if (r.carried) CHECK(r.slot_base == expect_base);
        const int base = r.slot_base;
        // the launches: {w0} (not carried), then groups of `group`; each counts the next group ahead,
        // the last one the next call's first group when the call speculates
        std::vector<std::pair<int, int>> launches;  // (first window, windows)
        if (!r.carried) launches.push_back({0, 1});
        for (int w = r.carried ? 0 : 1; w < nw; w += group) launches.push_back({w, group < nw - w ? group : nw - w});
        for (const auto& l : launches) {
          const int la0 = l.first + l.second, ahead_in_call = group < nw - la0 ? group : nw - la0;
          const int la = la0 < nw ? ahead_in_call : r.speculated ? (group < nw ? group : nw) : 0;
          std::set<int> used;
          for (int i = 0; i < l.second + la; ++i) used.insert(mdr::carry_slot(base, l.first + i));
          CHECK((int)used.size() == l.second + la);
        }
        expect_base = mdr::carry_slot(base, nw);
        if (r.speculated) {
          CHECK(c.v.carry().slot_base == expect_base);
          CHECK(c.v.carry().nw == (group < nw ? group : nw));
        }
      }
    }
}

}  // namespace

int main() {
  script_six_calls();
  script_drops();
  script_slots();
  if (failures) {
    std::fprintf(stderr, "carry_check: %d failure(s)\n", failures);
    return 1;
  }
  std::printf("carry_check: ok\n");
  return 0;
}
