// Owners of what libmi_phylo.so gets from the HIP runtime: device memory (Buffer), pinned host
// memory (PinnedArena, PinnedWord), events, a stream.  Each releases what it holds when it goes,
// so an early return leaks nothing.  No engine in here: mi_site_pattern.hip includes this alone.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace miphylo {
int fail(const std::string& msg);  // sets mi_last_error() (mi_phylo_engine.cpp)
// device memory owned by the Buffers of this process (mi_device_bytes_held)
extern std::atomic<int64_t> device_bytes_held;
}  // namespace miphylo

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t err__ = (expr);                                                              \
    if (err__ != hipSuccess)                                                                \
      return miphylo::fail(std::string("HIP error: ") + hipGetErrorString(err__) + " at " + \
                           __FILE__ + ":" + std::to_string(__LINE__));                      \
  } while (0)

// A device buffer that only ever grows.
struct Buffer {
  void* ptr = nullptr;
  size_t bytes = 0;
  Buffer() = default;
  Buffer(const Buffer&) = delete;
  Buffer& operator=(const Buffer&) = delete;
  ~Buffer() { release(); }
  int ensure(size_t need) {
    if (need <= bytes) return 0;
    release();
    HIP_TRY(hipMalloc(&ptr, need));
    bytes = need;
    miphylo::device_bytes_held += (int64_t)need;
    return 0;
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    detach();
  }
  // the allocation becomes the caller's, to free with hipFree
  void* detach() {
    void* p = ptr;
    miphylo::device_bytes_held -= (int64_t)bytes;
    ptr = nullptr;
    bytes = 0;
    return p;
  }
  template <typename T>
  T* as() const { return static_cast<T*>(ptr); }
};

// One device block cut into arrays, each starting on a 256-byte boundary: sizes first (base null: every
// pointer null, `at` the bytes needed), then the pointers.
struct Cutter {
  char* base;
  size_t at = 0;
  template <typename T>
  void take(T*& p, size_t count) {
    p = base ? reinterpret_cast<T*>(base + at) : nullptr;
    at += (std::max<size_t>(count, 1) * sizeof(T) + 255) & ~(size_t)255;
  }
};
// Synchronous copies of the creation and host-form paths; a null host pointer (an optional array) copies nothing.
inline int upload(void* dst, const void* src, size_t bytes) {
  if (src && bytes) HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return 0;
}
inline int download(void* dst, const void* src, size_t bytes) {
  if (dst && bytes) HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return 0;
}

// Pinned host staging for the host-pointer entry points: inputs are copied into it and
// DMA'd from there, outputs are DMA'd into it and copied out after the call's one
// synchronisation.  (hipMemcpyAsync on pageable memory is staged by the runtime, copy by
// copy and mostly synchronously: ~0.5 ms per call for 1000 DS1 trees, against ~0.1 ms.)
struct PinnedArena {
  char* ptr = nullptr;
  size_t bytes = 0, used = 0;
  struct Pending {
    void* host;
    const void* staged;
    size_t bytes;
  };
  std::vector<Pending> pending;
  PinnedArena() = default;
  PinnedArena(const PinnedArena&) = delete;
  PinnedArena& operator=(const PinnedArena&) = delete;
  ~PinnedArena() { release(); }
  // returns nullptr on failure; may synchronise `s` when it has to grow
  void* alloc(size_t need, hipStream_t s) {
    need = (need + 255) & ~(size_t)255;
    if (used + need > bytes) {
      // copies already issued from / into the old block must finish before it goes away;
      // pending outputs are delivered first
      if (hipStreamSynchronize(s) != hipSuccess) return nullptr;
      flush();
      const size_t want = std::max<size_t>(2 * (used + need), 1 << 20);
      release();
      if (hipHostMalloc(reinterpret_cast<void**>(&ptr), want, hipHostMallocDefault) != hipSuccess)
        return nullptr;
      bytes = want;
    }
    void* p = ptr + used;
    used += need;
    return p;
  }
  void flush() {  // after a synchronisation: hand the staged outputs to the caller
    for (const Pending& q : pending) memcpy(q.host, q.staged, q.bytes);
    pending.clear();
  }
  void reset() {
    pending.clear();
    used = 0;
  }
  void release() {
    if (ptr) (void)hipHostFree(ptr);
    ptr = nullptr;
    bytes = used = 0;
    pending.clear();
  }
};

// One handle of the HIP runtime, released through `Free` when its owner goes; reads as the
// handle it holds (filled in by the creating call through &x.h) and moves, never copies.
template <typename T, auto Free>
struct Owned {
  T h = nullptr;
  Owned() = default;
  Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
  ~Owned() {
    if (h) (void)Free(h);
  }
  operator T() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using Event = Owned<hipEvent_t, hipEventDestroy>;
using PinnedWord = Owned<int32_t*, hipHostFree>;  // what a copy lands in that the host reads next
