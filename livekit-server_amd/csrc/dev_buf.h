// dev_buf.h — an owning device buffer: pointer + element capacity in one
// move-only value, and the families of such buffers that grow together.  No HIP header: the two allocation functions below are
// defined by engine.cpp (hipMalloc / hipFree + the range registry) and by a
// malloc-backed fake in host_unit.cpp; a status is the hipError_t value as an
// int (0: success).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace lkf {

int dev_alloc(void **p, size_t bytes);  // *p = nullptr on failure
int dev_free(void *p);                  // p != nullptr

template <typename T>
class DevBuf {
 public:
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept : p_(o.p_), cap_(o.cap_) {
    o.p_ = nullptr;
    o.cap_ = 0;
  }
  DevBuf &operator=(DevBuf &&o) noexcept {
    if (this != &o) {
      (void)reset();
      p_ = o.p_;
      cap_ = o.cap_;
      o.p_ = nullptr;
      o.cap_ = 0;
    }
    return *this;
  }
  ~DevBuf() { (void)reset(); }

  operator T *() const { return p_; }
  T *get() const { return p_; }
  uint64_t cap() const { return cap_; }  // elements

  int reset() {
    const int r = p_ ? dev_free(p_) : 0;
    p_ = nullptr;
    cap_ = 0;
    return r;
  }
  // Exactly n elements (the fixed-size tables); an old buffer is freed first.
  // The capacity is recorded only once the allocation has succeeded: after a
  // failure the buffer is empty (null, capacity 0) and the next call retries.
  int alloc(uint64_t n) {
    (void)reset();
    void *q = nullptr;
    const int r = dev_alloc(&q, size_t(n ? n : 1) * sizeof(T));
    if (r) return r;
    p_ = static_cast<T *>(q);
    cap_ = n;
    return 0;
  }
  // Grows to max(n, floor) elements when n > cap(); the contents are not kept.
  int reserve(uint64_t n, uint64_t floor) { return n <= cap_ ? 0 : alloc(n > floor ? n : floor); }

 private:
  T *p_ = nullptr;
  uint64_t cap_ = 0;
};

// Frees every buffer of a family before any of them grows again.
template <typename... B>
void release_all(B &...b) {
  (void)(..., b.reset());
}

// A buffer of a scratch family (buffers that one call uses together): `need`
// elements now; when the family regrows it gets max(size, floor) elements,
// size = need unless given (headroom for the next, larger call).
template <typename T>
struct Want {
  DevBuf<T> &b;
  uint64_t need, size;
};
template <typename T>
Want<T> want(DevBuf<T> &b, uint64_t need, uint64_t floor, uint64_t size = 0) {
  if (!size) size = need;
  return {b, need, size > floor ? size : floor};
}

template <typename... T>
bool family_short(const Want<T> &...w) {
  return (... || (w.need > w.b.cap()));
}

// Frees the whole family, then allocates every buffer again in the order
// listed, none smaller than it was: calls that share a family with different
// shapes settle on one size instead of reallocating in turn.  Stops at the
// first failure and returns its status (the buffers behind it stay empty).
template <typename... T>
int regrow_family(Want<T>... w) {
  (void)(..., (w.size = w.size > w.b.cap() ? w.size : w.b.cap()));
  release_all(w.b...);
  int r = 0;
  (void)(... && ((r = w.b.alloc(w.size)) == 0));
  return r;
}

}  // namespace lkf
