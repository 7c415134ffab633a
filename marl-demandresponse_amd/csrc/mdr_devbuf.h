// mdr_devbuf.h — the owner of one block of device memory.  Host-only and free of HIP names, so its
// rules are checked on the CPU under a counting allocator (tests/devbuf_check.cpp).
// Alloc: static int alloc(void** p, size_t bytes) (0, or its error code); static void release(void* p).
#pragma once

#include <cstddef>

namespace mdr {

template <class T, class Alloc>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr, o.n_ = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_, n_ = o.n_;
      o.p_ = nullptr, o.n_ = 0;
    }
    return *this;
  }
  ~DevBuf() { reset(); }

  // Room for n elements; the contents are not kept.  Within the capacity nothing happens.  Otherwise
  // the old block is released FIRST (the greedy scratch of 16M houses is several hundred MB: the peak
  // must not double) and the capacity is recorded only once the allocator succeeded: a failed grow
  // leaves (null, 0), never a pointer or a capacity over freed memory.
  int reserve(size_t n) {
    if (n <= n_) return 0;
    reset();
    void* p = nullptr;
    if (int e = Alloc::alloc(&p, n * sizeof(T))) return e;
    p_ = static_cast<T*>(p), n_ = n;
    return 0;
  }
  void reset() {
    if (p_) Alloc::release(p_);
    p_ = nullptr, n_ = 0;
  }
  T* get() const { return p_; }
  size_t capacity() const { return n_; }  // in elements
  operator T*() const { return p_; }      // a launch site names the buffer as it named the pointer

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};

// Buffers sized together grow together, all or nothing: clear() empties every member and zeroes the
// unit's capacity, fill() reserves the members in order and returns the first error.  A failure
// anywhere leaves the whole unit empty, so the next call allocates again.
template <class Clear, class Fill>
int grow_unit(Clear clear, Fill fill) {
  clear();
  const int rc = fill();
  if (rc) clear();
  return rc;
}

}  // namespace mdr
