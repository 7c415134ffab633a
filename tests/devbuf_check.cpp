// devbuf_check.cpp — csrc/mdr_devbuf.h under a counting allocator (tests/test_devbuf_cpu.py builds and
// runs it, plain and under AddressSanitizer + UBSan).  The allocator keeps the set of live blocks,
// aborts on the release of an unknown or already released pointer, and fails the k-th allocation on
// request: the allocation-failure paths of the context (mdr_capi.hip), which no GPU test may provoke.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>

#include "mdr_devbuf.h"

namespace {

struct Counting {
  static std::set<void*>& live() { static std::set<void*> s; return s; }
  static int allocs, releases, fail_at;  // fail_at: the allocation (counted from 1) that fails; 0: none
  static long order;                     // +1 per event: the checks read releases-before-allocations from it
  static long last_alloc, last_release;
  static int alloc(void** p, size_t bytes) {
    ++allocs;
    last_alloc = ++order;
    if (fail_at && allocs == fail_at) return 2;  // (hipErrorOutOfMemory's value; any non-zero code)
    *p = std::malloc(bytes ? bytes : 1);
    live().insert(*p);
    return 0;
  }
  static void release(void* p) {
    if (!live().erase(p)) {
      std::fprintf(stderr, "release of a pointer that is not live: %p\n", p);
      std::abort();
    }
    ++releases;
    last_release = ++order;
    std::free(p);
  }
  static void arm(int k) { allocs = 0, fail_at = k; }
};
int Counting::allocs = 0, Counting::releases = 0, Counting::fail_at = 0;
long Counting::order = 0, Counting::last_alloc = 0, Counting::last_release = 0;

using Buf = mdr::DevBuf<double, Counting>;

int failures = 0;
#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                            \
    }                                                                        \
  } while (0)

void test_reserve() {
  Counting::arm(0);
  Buf b;
  CHECK(b.get() == nullptr && b.capacity() == 0);
  CHECK(b.reserve(0) == 0 && Counting::allocs == 0);  // nothing fits in nothing
  CHECK(b.reserve(100) == 0 && b.capacity() == 100 && Counting::live().size() == 1);
  double* p = b;
  const int a0 = Counting::allocs, r0 = Counting::releases;
  CHECK(b.reserve(100) == 0 && b.reserve(7) == 0);  // within capacity: the same block, no allocator call
  CHECK(b.get() == p && b.capacity() == 100 && Counting::allocs == a0 && Counting::releases == r0);
  p[99] = 1.0;  // (the sanitizer build checks the size)
  // a grow releases exactly once, and before it allocates
  CHECK(b.reserve(101) == 0 && b.capacity() == 101);
  CHECK(Counting::releases == r0 + 1 && Counting::allocs == a0 + 1 && Counting::last_release < Counting::last_alloc);
  CHECK(Counting::live().size() == 1);
  b.get()[100] = 1.0;
  b.reset();
  CHECK(b.get() == nullptr && b.capacity() == 0 && Counting::live().empty());
  b.reset();  // (idempotent)
}

void test_failed_grow() {
  Counting::arm(0);
  Buf b;
  CHECK(b.reserve(64) == 0);
  Counting::arm(1);
  CHECK(b.reserve(128) == 2);  // the allocator's code comes back
  CHECK(b.get() == nullptr && b.capacity() == 0 && Counting::live().empty());  // empty, the old block released
  Counting::arm(0);
  // the smaller request that the old capacity (64) would have let through allocates
  CHECK(b.reserve(32) == 0 && b.get() != nullptr && b.capacity() == 32 && Counting::allocs == 1);
}

void test_moves() {
  Counting::arm(0);
  Buf a;
  CHECK(a.reserve(8) == 0);
  double* p = a;
  Buf b(std::move(a));
  CHECK(a.get() == nullptr && a.capacity() == 0 && b.get() == p && b.capacity() == 8);
  Buf c;
  CHECK(c.reserve(4) == 0);
  const int r0 = Counting::releases;
  c = std::move(b);  // c's own block is released, b's moves in
  CHECK(Counting::releases == r0 + 1 && c.get() == p && c.capacity() == 8 && b.get() == nullptr && b.capacity() == 0);
  Buf& cr = c;
  c = std::move(cr);  // (self-move keeps the block)
  CHECK(c.get() == p && Counting::live().size() == 1);
}  // a, b, c destroyed: one release, not three

// A unit as the context has them (greedy_scratch's shape): members that are sized together, one
// capacity, grown by mdr::grow_unit.
struct Unit {
  Buf key, idx, tmp, win;
  long cap = 0;
  void clear() {
    key.reset(), idx.reset(), tmp.reset(), win.reset();
    cap = 0;
  }
  bool empty() const { return !key.get() && !idx.get() && !tmp.get() && !win.get() && cap == 0; }
  // 0 when n fits, else the whole unit anew for n
  int ensure(long n) {
    if (cap >= n) return 0;
    const int rc = mdr::grow_unit([&] { clear(); }, [&]() -> int {
      if (int e = key.reserve(n)) return e;
      if (int e = idx.reserve(n)) return e;
      if (int e = tmp.reserve(2 * n)) return e;
      return win.reserve(16);
    });
    if (!rc) cap = n;
    return rc;
  }
};

void test_unit_failure_at_each_position() {
  for (int k = 1; k <= 4; ++k) {
    Counting::arm(0);
    Unit u;
    CHECK(u.ensure(1000) == 0 && u.cap == 1000 && Counting::live().size() == 4);
    Counting::arm(k);  // the k-th allocation of the regrow fails
    CHECK(u.ensure(2000) != 0);
    CHECK(u.empty() && Counting::live().empty());  // wholly empty: nothing dangling, no stale capacity
    Counting::arm(0);
    // the defect this replaces: the old capacity (1000) let a smaller request "fit" over freed members
    CHECK(u.ensure(500) == 0 && Counting::allocs == 4 && u.cap == 500 && u.key.get() && u.win.get());
    CHECK(u.ensure(2000) == 0 && u.cap == 2000 && Counting::live().size() == 4);  // and the retry succeeds
  }
  // a failure on the very first growth (nothing to release) leaves the same empty unit
  Counting::arm(2);
  Unit u;
  CHECK(u.ensure(10) != 0 && u.empty() && Counting::live().empty());
}

}  // namespace

int main() {
  test_reserve();
  test_failed_grow();
  test_moves();
  test_unit_failure_at_each_position();
  CHECK(Counting::live().empty());  // every block released exactly once (a second release aborts)
  if (failures) {
    std::fprintf(stderr, "devbuf_check: %d check(s) failed\n", failures);
    return 1;
  }
  std::puts("devbuf_check: ok");
  return 0;
}
