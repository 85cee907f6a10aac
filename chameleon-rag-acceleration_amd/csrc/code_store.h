// The flat indexes' code store.
// What IndexPQ, IndexScalarQuantizer, IndexBinaryFlat and IndexFlat share: one device image of
// fixed-size code rows [ntotal][row_bytes] that grows geometrically (with `slack` bytes
// behind it where the scan reads past a row), the label of a code being its position;
// the handle's own stream; and the ordering of device calls on different streams one
// after the other (one workspace per handle, StreamOrder).
#pragma once
#include <memory>

#include "host_common.h"

namespace chivf {

struct CodeStore : StreamOrder {
  const char* const name;  // the Faiss index, for messages
  int device = 0;
  int64_t ntotal = 0, cap = 0;      // codes in the image, rows allocated
  size_t row_bytes = 0, slack = 0;  // bytes per image row, bytes allocated behind the last row
  DevBuf d_codes;
  DevBuf w_x;  // staging of host rows
  hipStream_t stream = nullptr;
  std::mutex mu;

  explicit CodeStore(const char* index_name) : name(index_name) {}
  ~CodeStore() {
    if (stream) (void)hipStreamDestroy(stream);
  }

  uint8_t* row(int64_t i) const { return d_codes.as<uint8_t>() + (size_t)i * row_bytes; }

  // room for n more codes: the image doubles (at least) when it is full
  void reserve(int64_t n, hipStream_t s) {
    require(ntotal + n < (int64_t)INT32_MAX, std::string(name) + " holds at most 2^31 - 2 codes");
    if (ntotal + n <= cap) return;
    quiesce();
    const int64_t ncap = std::max<int64_t>({ntotal + n, 2 * cap, 1024});
    grow(d_codes, (size_t)ncap * row_bytes + slack, (size_t)ntotal * row_bytes, s);
    cap = ncap;
  }

  // b reallocated at nbytes, its first keep bytes copied over on s; returns when they are
  static void grow(DevBuf& b, size_t nbytes, size_t keep, hipStream_t s) {
    DevBuf nb;
    nb.ensure(nbytes);
    if (keep) {
      HIPCHECK(hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, s));
      HIPCHECK(hipStreamSynchronize(s));
    }
    b.swap(nb);
  }

  // n host rows [n][row_bytes] behind the image; returns when they are in place
  void append_rows(int64_t n, const uint8_t* codes) {
    reserve(n, stream);
    quiesce();
    HIPCHECK(hipMemcpyAsync(row(ntotal), codes, (size_t)n * row_bytes, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    ntotal += n;
  }

  // the first out_bytes (<= row_bytes) of the rows [i0, i0 + n) to the host
  void read_rows(int64_t i0, int64_t n, uint8_t* out, size_t out_bytes) {
    quiesce();
    if (out_bytes == row_bytes)
      HIPCHECK(hipMemcpyAsync(out, row(i0), (size_t)n * row_bytes, hipMemcpyDeviceToHost, stream));
    else
      HIPCHECK(hipMemcpy2DAsync(out, out_bytes, row(i0), row_bytes, out_bytes, n, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }

  void reset() {
    quiesce();
    d_codes.release();
    ntotal = cap = 0;
  }

  // rows per chunk of n host rows of in_bytes each that pass through a staging buffer
  static int64_t host_rows(int64_t n, size_t in_bytes) {
    return scratch_rows(n, in_bytes);
  }

  // n host rows of in_bytes each, staged chunk by chunk in w_x; add(c) puts the c staged
  // rows behind the image on the handle's stream and returns when they are in place
  template <class F>
  void add_host(int64_t n, const void* x, size_t in_bytes, F add) {
    const int64_t rows = host_rows(n, in_bytes);
    quiesce();
    w_x.ensure((size_t)rows * in_bytes);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      HIPCHECK(hipMemcpyAsync(w_x.p, (const uint8_t*)x + (size_t)r0 * in_bytes, (size_t)c * in_bytes,
                              hipMemcpyHostToDevice, stream));
      add(c);
    }
  }
};

// the end of every *_create: the device checked, the handle's stream and event made on it
template <class H>
void open_store(std::unique_ptr<H> h, int device, H** out) {
  int ndev = 0;
  HIPCHECK(hipGetDeviceCount(&ndev));
  require(device >= 0 && device < ndev, "device ordinal out of range");
  DeviceGuard g(device);
  h->device = device;
  HIPCHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  h->create();
  *out = h.release();
}

// the search arguments of the flat indexes (one that needs no training passes true)
inline void check_flat_search_args(bool trained, int64_t n, const void* x, int k, const void* D, const void* I) {
  require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
  require(trained, "index is not trained");
  require(n >= 0, "negative query count");
  require(n == 0 || (x && D && I), "null x / D / I");
}

}  // namespace chivf
