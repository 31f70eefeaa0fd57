// hip_own.h — owners of the engine's other HIP resources (events, streams,
// graph execs, page-locked host memory).  They are members of the engine and
// its batch contexts, never copied or moved.  Each converts to its raw
// handle, so the HIP calls and launch_* keep their argument lists; the
// destructors are the only places that release them.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

namespace lkf {

// Base of the handle owners: one raw handle, never copied or moved.
template <typename H>
struct Owned {
  H h = nullptr;
  Owned() = default;
  Owned(const Owned &) = delete;
  Owned &operator=(const Owned &) = delete;
  operator H() const { return h; }
  H get() const { return h; }
};

struct Event : Owned<hipEvent_t> {
  ~Event() { reset(); }
  hipError_t create(bool timing) {
    reset();
    return timing ? hipEventCreate(&h) : hipEventCreateWithFlags(&h, hipEventDisableTiming);
  }
  void reset() {
    if (h) (void)hipEventDestroy(h);
    h = nullptr;
  }
};

// A stream the engine created (put(): the hipStreamCreate* out-parameter) or
// a non-owning second name of another one (view()).
struct Stream : Owned<hipStream_t> {
  bool owned = false;
  ~Stream() { reset(); }
  hipStream_t *put() {
    reset();
    owned = true;
    return &h;
  }
  void view(const Stream &o) {
    reset();
    h = o.h;
  }
  void reset() {
    if (h && owned) (void)hipStreamDestroy(h);
    h = nullptr;
    owned = false;
  }
};

struct GraphExec : Owned<hipGraphExec_t> {
  ~GraphExec() { reset(); }
  hipError_t destroy() {
    const hipError_t r = h ? hipGraphExecDestroy(h) : hipSuccess;
    h = nullptr;
    return r;
  }
  void reset() { (void)destroy(); }
};

// A stage of lkf_run captured as a graph, with the topology epoch it was
// captured for (epoch 0: none, re-captured by its next use).
struct StageGraph {
  GraphExec exec;
  uint64_t epoch = 0;
};

// Page-locked, CPU-cached host staging (aligned_alloc + hipHostRegister) with
// its device mapping.
struct StagePair {
  uint8_t *host = nullptr, *dev = nullptr;
  StagePair() = default;
  StagePair(const StagePair &) = delete;
  StagePair &operator=(const StagePair &) = delete;
  ~StagePair() { reset(); }
  hipError_t alloc(size_t n) {
    reset();
    const size_t bytes = (n + 4095) & ~size_t(4095);
    void *p = std::aligned_alloc(4096, bytes);
    if (!p) return hipErrorOutOfMemory;
    hipError_t r = hipHostRegister(p, bytes, hipHostRegisterMapped);
    void *d = nullptr;
    if (r == hipSuccess && (r = hipHostGetDevicePointer(&d, p, 0)) != hipSuccess) (void)hipHostUnregister(p);
    if (r != hipSuccess) {
      std::free(p);
      return r;
    }
    host = static_cast<uint8_t *>(p);
    dev = static_cast<uint8_t *>(d);
    return hipSuccess;
  }
  void reset() {
    if (host) {
      (void)hipHostUnregister(host);
      std::free(host);
    }
    host = dev = nullptr;
  }
};

// Pinned host memory (hipHostMalloc): the drains' bounce buffer.
struct PinnedBuf {
  uint8_t *p = nullptr;
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf &) = delete;
  PinnedBuf &operator=(const PinnedBuf &) = delete;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  hipError_t alloc(size_t bytes) { return hipHostMalloc(reinterpret_cast<void **>(&p), bytes, hipHostMallocDefault); }
};

}  // namespace lkf
