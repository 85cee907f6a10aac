// What every handle of libivfpq.so's host side uses: HIP error checks, device buffers,
// the scratch bounds, the library's one error string and the opening of a C-ABI entry
// point.  Host code only (the kernels do not include it).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <mutex>
#include <stdexcept>
#include <string>
#include <utility>

#include "ivfpq_kernels.h"  // kMaxK

namespace chivf {

#define HIPCHECK(x)                                                                          \
  do {                                                                                       \
    hipError_t e_ = (x);                                                                     \
    if (e_ != hipSuccess) throw std::runtime_error(std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

inline void require(bool ok, const std::string& msg) {
  if (!ok) throw std::runtime_error(msg);
}

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  void ensure(size_t b) {
    if (b <= bytes && p) return;
    release();
    if (b == 0) b = 16;
    HIPCHECK(hipMalloc(&p, b));
    bytes = b;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
  void swap(DevBuf& o) {
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
};

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    HIPCHECK(hipGetDevice(&prev));
    if (prev != dev) HIPCHECK(hipSetDevice(dev));
  }
  ~DeviceGuard() {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur != prev && prev >= 0) (void)hipSetDevice(prev);
  }
};

constexpr size_t kChunkBytes = size_t(256) << 20;    // bound for [rows][cols] fp32 scratch
constexpr size_t kPartialBytes = size_t(2048) << 20;  // bound for a chunk's per-wave partial top-k lists
// from this nlist on, the coarse quantizer never writes the key matrix (r03 A/B at
// C2, nlist 1024: segmented 22.5 + 8.5 us + a separate T3 launch 13.0 us vs key
// matrix 17.8 + 10.0 us with T3 in the same launch)
constexpr int kSegmentedNlist = 8192;

// the calling thread's last failure, of whichever index (ivfpq_last_error)
inline thread_local std::string g_err;

template <class F>
int guarded(F&& f) {
  try {
    g_err.clear();
    f();
    return 0;
  } catch (const std::exception& e) {
    g_err = e.what();
  } catch (...) {
    g_err = "unknown error";
  }
  return -1;
}

template <class H>
void check_handle(const H* h) {
  require(h != nullptr, "null index handle");
}

// The common opening of a C-ABI entry point: f runs with failures caught, the handle
// checked, its mutex held and its device current.
template <class H, class F>
int with_handle(H* h, F&& f) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    f();
  });
}

// every *_free: the handle's work drained on its device, then the handle deleted
template <class H>
int free_handle(H* h) {
  return guarded([&] {
    if (!h) return;
    DeviceGuard g(h->device);
    (void)hipStreamSynchronize(h->stream);
    h->quiesce();
    delete h;
  });
}

// Device calls of a handle with one workspace, ordered one after the other across
// streams: every call records `done` on its stream, the next one on another stream
// waits for it, and whatever frees or rewrites the buffers synchronizes on it first.
struct StreamOrder {
  hipEvent_t done = nullptr;
  hipStream_t done_stream = nullptr;
  bool done_pending = false;

  StreamOrder() = default;
  StreamOrder(const StreamOrder&) = delete;
  StreamOrder& operator=(const StreamOrder&) = delete;
  ~StreamOrder() {
    if (done) (void)hipEventDestroy(done);
  }
  void create() { HIPCHECK(hipEventCreateWithFlags(&done, hipEventDisableTiming)); }
  void order_after(hipStream_t s) {
    if (done_pending && done_stream != s) HIPCHECK(hipStreamWaitEvent(s, done, 0));
  }
  void mark_done(hipStream_t s) {
    HIPCHECK(hipEventRecord(done, s));
    done_stream = s;
    done_pending = true;
  }
  void quiesce() {
    if (done_pending) HIPCHECK(hipEventSynchronize(done));
    done_pending = false;
  }
};

// The search arguments of the IVF indexes (the flat indexes check in another order, with
// other words: code_store.h).
inline void check_search_args(bool trained, int64_t n, int k) {
  require(trained, "index is not trained");
  require(n >= 0, "n must be >= 0");
  require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
}

}  // namespace chivf
