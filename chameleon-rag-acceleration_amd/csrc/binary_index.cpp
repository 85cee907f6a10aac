// Flat binary codes (IndexBinaryFlat) behind the C-ABI of include/ivfpq.h.
// faiss.IndexBinaryFlat: uint8 codes of d bits, every code compared with every query by
// Hamming distance and the k smallest (distance, label) selected by counting
// (binary_flat.hip).  The codes live in a CodeStore of stride bytes per row (rows padded
// with zero bytes to whole loads).
#include "binary_flat.h"
#include "code_store.h"
#include "ivfpq.h"

using namespace chivf;

struct ivfpq_bin_index : CodeStore {
  int d = 0, code_size = 0, stride = 0;  // stride = row_bytes: a row padded to whole loads
  DevBuf w_D, w_I, p_qw, p_hist, p_T, p_quota;

  ivfpq_bin_index() : CodeStore("IndexBinaryFlat") {}

  // pad n device-resident codes [n][code_size] behind the image; returns when they are in place
  void add_dev(int64_t n, const uint8_t* xd, hipStream_t s) {
    reserve(n, s);
    order_after(s);
    launch_bin_pad_rows(xd, n, code_size, stride, d_codes.as<uint32_t>() + (size_t)ntotal * (stride / 4), s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    ntotal += n;
  }

  // n device-resident queries -> D, I (device), all on s
  void search_dev(int64_t n, const uint8_t* xd, int k, int32_t* D, int64_t* I, hipStream_t s) {
    if (n == 0) return;
    order_after(s);
    if (ntotal == 0) {
      launch_bin_fill_empty(D, I, n * k, s);
      HIPCHECK(hipGetLastError());
      mark_done(s);
      return;
    }
    const BinPlan pl = bin_plan(d, ntotal, n);
    const int64_t qc = std::min(pl.qc, n);
    const int64_t nblocks = (qc + pl.QB - 1) / pl.QB;
    p_qw.ensure((size_t)nblocks * pl.QB * pl.stride);
    p_hist.ensure(sizeof(uint32_t) * (size_t)qc * pl.Sg * (d + 1));
    p_T.ensure(sizeof(int32_t) * qc);
    p_quota.ensure(sizeof(uint32_t) * (size_t)qc * pl.Sg);
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      BinSearchArgs a;
      a.x = xd + q0 * code_size;
      a.nq = std::min(qc, n - q0);
      a.d = d;
      a.codes = d_codes.as<uint32_t>();
      a.nb = ntotal;
      a.k = k;
      a.qw = p_qw.as<uint32_t>();
      a.hist = p_hist.as<uint32_t>();
      a.T = p_T.as<int32_t>();
      a.quota = p_quota.as<uint32_t>();
      a.D = D + q0 * k;
      a.I = I + q0 * k;
      launch_bin_search(a, pl, s);
      HIPCHECK(hipGetLastError());
    }
    mark_done(s);
  }

  void search_host(int64_t n, const uint8_t* x, int k, int32_t* D, int64_t* I) {
    if (n == 0) return;
    quiesce();
    w_x.ensure((size_t)n * code_size);
    w_D.ensure(sizeof(int32_t) * n * k);
    w_I.ensure(sizeof(int64_t) * n * k);
    HIPCHECK(hipMemcpyAsync(w_x.p, x, (size_t)n * code_size, hipMemcpyHostToDevice, stream));
    search_dev(n, w_x.as<uint8_t>(), k, w_D.as<int32_t>(), w_I.as<int64_t>(), stream);
    HIPCHECK(hipMemcpyAsync(D, w_D.p, sizeof(int32_t) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipMemcpyAsync(I, w_I.p, sizeof(int64_t) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
};

namespace {
void check_bin_d(int d) {
  require(d >= 8 && d <= kBinMaxD && d % 8 == 0,
          "IndexBinaryFlat: d must be a multiple of 8 in [8, 2048] (d = " + std::to_string(d) + ")");
}
}  // namespace

extern "C" {

int ivfpq_bin_create(int d, int device, ivfpq_bin_index** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    check_bin_d(d);
    auto h = std::make_unique<ivfpq_bin_index>();
    h->d = d;
    h->code_size = d / 8;
    h->stride = bin_stride(h->code_size);
    h->row_bytes = (size_t)h->stride;
    open_store(std::move(h), device, out);
  });
}

int ivfpq_bin_free(ivfpq_bin_index* h) { return free_handle(h); }

int ivfpq_bin_reset(ivfpq_bin_index* h) {
  return with_handle(h, [&] { h->reset(); });
}

int ivfpq_bin_add(ivfpq_bin_index* h, int64_t n, const uint8_t* x) {
  return with_handle(h, [&] {
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_host(n, x, (size_t)h->code_size, [&](int64_t c) { h->add_dev(c, h->w_x.as<uint8_t>(), h->stream); });
  });
}

int ivfpq_bin_add_device(ivfpq_bin_index* h, int64_t n, const uint8_t* x, void* stream) {
  return with_handle(h, [&] {
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, (hipStream_t)stream);
  });
}

// (the searches check their arguments before the handle)
int ivfpq_bin_search(ivfpq_bin_index* h, int64_t n, const uint8_t* x, int k, int32_t* D, int64_t* I) {
  return guarded([&] {
    check_flat_search_args(true, n, x, k, D, I);  // nothing to train
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->search_host(n, x, k, D, I);
  });
}

int ivfpq_bin_search_device(ivfpq_bin_index* h, int64_t n, const uint8_t* x, int k, int32_t* D, int64_t* I,
                            void* stream) {
  return guarded([&] {
    check_flat_search_args(true, n, x, k, D, I);  // nothing to train
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->search_dev(n, x, k, D, I, (hipStream_t)stream);
  });
}

int64_t ivfpq_bin_ntotal(const ivfpq_bin_index* h) { return h ? h->ntotal : -1; }

int ivfpq_bin_get_dims(const ivfpq_bin_index* h, int* d, int* code_size) {
  return guarded([&] {
    check_handle(h);
    if (d) *d = h->d;
    if (code_size) *code_size = h->code_size;
  });
}

int ivfpq_bin_get_codes(ivfpq_bin_index* h, int64_t i0, int64_t n, uint8_t* out) {
  return with_handle(h, [&] {
    require(i0 >= 0 && n >= 0 && i0 + n <= h->ntotal, "code range outside [0, ntotal)");
    if (n == 0) return;
    require(out != nullptr, "null output pointer");
    h->read_rows(i0, n, out, (size_t)h->code_size);  // the rows without their pad bytes
  });
}

int ivfpq_bin_get_plan(int d, int64_t ntotal, int64_t nq, int k, int* stride, int* query_block, int* segments,
                       int64_t* segment_rows, int64_t* query_chunk) {
  return guarded([&] {
    check_bin_d(d);
    require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
    require(ntotal >= 0 && ntotal < (int64_t)INT32_MAX && nq >= 0, "ntotal / nq out of range");
    const BinPlan pl = bin_plan(d, ntotal, nq);
    if (stride) *stride = pl.stride;
    if (query_block) *query_block = pl.QB;
    if (segments) *segments = pl.Sg;
    if (segment_rows) *segment_rows = pl.seg_rows;
    if (query_chunk) *query_chunk = pl.qc;
  });
}

}  // extern "C"
