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

#include "flat_scan.h"      // FlatScanPlan
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

// ---- how the host cuts a batch ("Host-side splits") ------------------------
// Every loop that takes a batch chunk by chunk asks one of these for its chunk, and so
// does the getter that reports the cut to a test (ivfpq_*_get_*): host arithmetic only.

// rows of n that pass at a time through a scratch buffer of kChunkBytes, row_bytes each
inline int64_t scratch_rows(int64_t n, size_t row_bytes) {
  return std::max<int64_t>(1, std::min<int64_t>(n, (int64_t)(kChunkBytes / row_bytes)));
}

// queries whose S sorted partial lists of k entries (12 bytes per entry, and the first merge
// round's output) stay within kPartialBytes, their count within the merge's 32-bit indexing
inline int64_t partial_list_queries(int S, int k) {
  const size_t part_q = (size_t)S * k * 12 * 2;
  return std::max<int64_t>(
      1, std::min<int64_t>((int64_t)(kPartialBytes / part_q), (int64_t)(INT32_MAX / 2) / ((int64_t)S * k)));
}

// the queries of one launch of the flat index's fused scan (IndexFlat's searches, the k-means
// assignment at k = 1) and its plan: the partial lists within kPartialBytes, their count
// within the merge's 32-bit indexing
inline int64_t flat_query_chunk(int64_t n, int64_t nb, int k, int64_t force, FlatScanPlan* out) {
  int64_t qc = std::max<int64_t>(1, std::min<int64_t>(n, 1 << 16));
  FlatScanPlan pl = flat_scan_plan(qc, nb, k, force);
  while (true) {
    const int64_t lim = partial_list_queries(pl.S, k);
    if (qc <= lim) break;
    qc = std::max<int64_t>(1, std::min(lim, qc / 2));
    pl = flat_scan_plan(qc, nb, k, force);  // fewer query tiles: more ranges
  }
  if (out) *out = pl;
  return qc;
}

// queries per chunk of a search whose scan leaves S partial lists per query (IndexScalarQuantizer)
inline int64_t partial_query_chunk(int64_t n, int S, int k) {
  return std::max<int64_t>(1, std::min<int64_t>(n, partial_list_queries(S, k)));
}

// queries per chunk of an IVF list-scan search (ivf_lists.h): the [c][nlist] coarse keys, buckets
// and what the row type keeps per entry (entry_bytes in all) within kChunkBytes, the partial
// lists as above, and where residual queries are kept their [c][np][d] floats within kChunkBytes
inline int64_t ivf_query_chunk(int64_t n, int nlist, size_t entry_bytes, int S, int k, int np, int d,
                               bool resid_queries) {
  int64_t qc = std::min<int64_t>({n, (int64_t)(kChunkBytes / ((size_t)nlist * entry_bytes)), partial_list_queries(S, k)});
  if (resid_queries) qc = std::min<int64_t>(qc, (int64_t)(kChunkBytes / (sizeof(float) * np * d)));
  return std::max<int64_t>(1, qc);
}

// queries per chunk of an IVF-PQ search: the [c][nlist] keys, T3 ([c][M][ksub]) and the buckets of
// the handle's nloc lists within kChunkBytes; the per-wave partial lists ([c][np][4][k] 16-byte
// records: 64 bytes per entry and query) within kPartialBytes, so large k still runs whole
// 1024-query batches (C3, k = 1000, nprobe 32: 2 MB per query)
inline int64_t ivfpq_query_chunk(int64_t n, int nlist, int M, int ksub, int nloc, int np, int k) {
  const size_t per_q = std::max({(size_t)nlist * 4, (size_t)M * ksub * 4, (size_t)std::max(nloc, 1) * 16});
  return std::max<int64_t>(
      1, std::min<int64_t>({n, (int64_t)(kChunkBytes / per_q), (int64_t)(kPartialBytes / ((size_t)np * part_stride(k) * 64))}));
}

// rows per pass of an IVF add or training pass: the [rows][nlist] coarse keys within kChunkBytes
// (2^18 rows where the coarse quantizer writes no key matrix), and a [rows][d] fp32 staging
// buffer where the pass has one
inline int64_t ivf_pass_rows(int64_t n, int nlist, int d, bool staged) {
  int64_t rows = nlist >= kSegmentedNlist ? (int64_t)1 << 18 : (int64_t)(kChunkBytes / ((size_t)nlist * 4));
  if (staged) rows = std::min<int64_t>(rows, (int64_t)(kChunkBytes / (sizeof(float) * d)));
  return std::max<int64_t>(1, std::min(n, rows));
}

// rows per pass of a k-means assignment: the [rows][k] fp32 distances within kChunkBytes
inline int64_t kmeans_assign_rows(int64_t n, int k) { return scratch_rows(n, (size_t)k * 4); }

// queries per chunk of the stateless exact search: the [c][nb] fp32 distances within kChunkBytes
inline int64_t flat_search_query_chunk(int64_t n, int64_t nb) {
  return scratch_rows(n, (size_t)std::max<int64_t>(nb, 1) * 4);
}

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
