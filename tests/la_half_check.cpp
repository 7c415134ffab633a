// la_half_check.cpp — the two halves of group mask rows across launches and call boundaries
// (csrc/mdr_validity.h: group_half, group_launches, CarriedCount::half) on the CPU.
// A model of the grouped direct sequence over the real Validity, not mdr_capi.hip's own code
// (tests/test_la_order_gpu.py runs that): every launch must read the half its windows' rows were
// written to and write the other one, within a call and across carried call boundaries, and every
// transition that ends a carried count must leave the next call at half 0.
#include <cstdio>
#include <cstdlib>

#include "mdr_validity.h"

using mdr::CarriedCount;
using mdr::Validity;

#define CHECK(c)                                                        \
  do {                                                                  \
    if (!(c)) {                                                         \
      std::printf("la_half_check: %s:%d: %s\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                     \
    }                                                                   \
  } while (0)

namespace {

int g_stream_tag;
const void* const kStream = &g_stream_tag;

// the device as the launches leave it: which group's rows each half holds (-1: none of this model's)
struct Rows {
  long in_half[2] = {-1, -1};
};

// one direct grouped call of nw windows in groups of G from tick0, as mdr_rollout issues it
struct Call {
  int n, nw, G;
};

// `next`: the id of the group the next group launch steps (ids number the groups of the whole run)
void run_call(Validity& v, Rows& dev, const Call& c, uint64_t tick0, long& next, bool speculate) {
  const bool carried = v.carry_matches(c.n, 1, tick0, 32, c.G, kStream);
  int half_in = 0;
  if (carried) {
    half_in = v.carry().half;
    v.carry_consumed();
    CHECK(v.carry().half == 0);
  } else {
    // the count kernel and the KA launch: it steps window 0 from the count kernel's rows and its
    // lookahead writes the next group's rows to half 0
    v.drop_carry();
    next += 1000;  // (nothing counted earlier is this call's)
    if (c.nw > 1 || speculate) dev.in_half[0] = next;
  }
  const int L = mdr::group_launches(carried, c.nw, c.G);
  int k = 0;
  for (int w = carried ? 0 : 1; w < c.nw; w += c.G, ++k) {
    const int rd = mdr::group_half(carried, half_in, k), wr = 1 - rd;
    CHECK(rd == 0 || rd == 1);
    CHECK(dev.in_half[rd] == next);  // this launch's windows' rows are in the half it reads
    const bool last = w + c.G >= c.nw;
    if (!last || speculate) dev.in_half[wr] = next + 1;  // the lookahead writes the other half
    next += 1;
  }
  CHECK(k == L);
  if (speculate) {
    CarriedCount r{};
    r.on = true, r.n = c.n, r.mode = 1, r.tick0 = tick0 + (uint64_t)c.n, r.window = 32, r.group = c.G;
    r.nw = c.nw < c.G ? c.nw : c.G;
    r.stream = kStream;
    r.half = mdr::group_half(carried, half_in, L);
    CHECK(dev.in_half[r.half] == next);  // the record names the half that holds the next call's first group
    v.carry_counted(r);
  }
}

void halves_alternate() {
  for (int h = 0; h < 2; ++h)
    for (int k = 0; k < 9; ++k) {
      CHECK(mdr::group_half(false, h, k) == (k & 1));  // a plain call starts at half 0 whatever the record said
      CHECK(mdr::group_half(true, h, k) == ((h + k) & 1));
      CHECK(mdr::group_half(true, h, k) != mdr::group_half(true, h, k + 1));
    }
  for (int G = 1; G <= mdr::kCarryGroup; ++G)
    for (int nw = 1; nw <= 20; ++nw) {
      int plain = 0, carried = 0;
      for (int w = 1; w < nw; w += G) ++plain;
      for (int w = 0; w < nw; w += G) ++carried;
      CHECK(mdr::group_launches(false, nw, G) == plain);
      CHECK(mdr::group_launches(true, nw, G) == carried);
    }
}

// twenty consecutive calls of every shape: the first counts its own window, the second speculates, the
// rest are carried; the half travels in the record
void carried_across_calls() {
  for (int G = 1; G <= mdr::kCarryGroup; ++G)
    for (int nw = 1; nw <= 10; ++nw) {
      Validity v;
      Rows dev;
      long group = 0;
      uint64_t tick = 100;
      const Call c{nw * 32, nw, G};
      for (int call = 0; call < 20; ++call) {
        const bool had = v.carry().on;
        run_call(v, dev, c, tick, group, call >= 1);
        CHECK(call < 2 || had);  // (carried from the third call on)
        tick += (uint64_t)c.n;
      }
      CHECK(v.carry_counters().speculated == 19 && v.carry_counters().consumed == 18);
    }
}

CarriedCount armed(int half) {
  CarriedCount r{};
  r.on = true, r.n = 128, r.mode = 1, r.tick0 = 7, r.window = 32, r.group = 4, r.nw = 4, r.stream = kStream;
  r.half = half;
  return r;
}

void reset_by_every_drop() {
  {
    Validity v;
    v.carry_counted(armed(1));
    CHECK(v.carry().on && v.carry().half == 1);
    v.state_may_change();
    CHECK(!v.carry().on && v.carry().half == 0 && v.carry_counters().dropped == 1);
  }
  {
    Validity v;
    v.carry_counted(armed(1));
    v.state_may_change(true);  // mdr_rollout itself: it settles the record once its arguments are checked
    CHECK(v.carry().on && v.carry().half == 1);
    v.drop_carry();
    CHECK(!v.carry().on && v.carry().half == 0);
  }
  {
    Validity v;
    v.carry_counted(armed(1));
    v.params_replaced();
    CHECK(!v.carry().on && v.carry().half == 0 && v.carry_counters().dropped == 1);
  }
  {
    Validity v;
    v.carry_counted(armed(1));
    v.state_replaced();
    CHECK(!v.carry().on && v.carry().half == 0);
  }
  {
    Validity v;
    v.carry_counted(armed(1));
    v.sequence_failed();
    CHECK(!v.carry().on && v.carry().half == 0 && v.carry_counters().dropped == 1);
  }
  {
    Validity v;
    v.carry_counted(armed(1));
    {
      mdr::Sequence seq(v, mdr::Sequence::kRollout);  // left without ok(): a failure
    }
    CHECK(!v.carry().on && v.carry().half == 0);
  }
  {  // a call that does not match the record starts at half 0
    Validity v;
    Rows dev;
    long group = 0;
    v.carry_counted(armed(1));
    run_call(v, dev, Call{96, 3, 4}, 1000, group, false);
    CHECK(!v.carry().on && v.carry().half == 0 && dev.in_half[0] >= 0);
  }
}

}  // namespace

int main() {
  halves_alternate();
  carried_across_calls();
  reset_by_every_drop();
  std::printf("la_half_check: ok\n");
  return 0;
}
