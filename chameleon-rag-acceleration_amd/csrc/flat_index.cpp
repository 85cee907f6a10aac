// Flat fp32 rows (IndexFlat) behind the C-ABI of include/ivfpq.h.
// faiss.IndexFlat / IndexFlatL2 / IndexFlatIP: the raw vectors, every row compared with
// every query (flat_scan.hip).  The rows live in a CodeStore of 4 d bytes per row; their
// |y|^2 (launch_row_norms' tree order) are computed once, when the rows are added, and kept
// beside the image.  Every k runs the fused scan: no distance is written to memory.
#include "code_store.h"
#include "flat_scan.h"
#include "ivf_flat.h"  // launch_fill_empty
#include "ivfpq.h"
#include "ivfpq_test.h"

using namespace chivf;

struct ivfpq_flat_index : CodeStore {
  int d = 0, metric = IVFPQ_METRIC_L2;
  DevBuf d_norms;              // [cap] |y|^2 of the image's rows
  int64_t norms_cap = 0;
  int64_t rows_from_host = 0;  // rows copied from the host since create (ivfpq_flat_index_get_stats)
  int64_t reallocs = 0;        // times the image was reallocated
  int64_t range_rows = 0;      // > 0: the row range of a scan workgroup (ivfpq_flat_index_set_range_rows)
  DevBuf w_xn, w_D, w_I, p_tau, p_partD, p_partI, p_tmpD, p_tmpI;

  ivfpq_flat_index() : CodeStore("IndexFlat") {}
  bool ip() const { return metric == IVFPQ_METRIC_INNER_PRODUCT; }
  float* base() const { return d_codes.as<float>(); }

  // room for n more rows in the image and the norms beside it
  void reserve_rows(int64_t n, hipStream_t s) {
    const int64_t before = cap;
    reserve(n, s);
    if (cap != before) reallocs++;
    if (cap <= norms_cap) return;
    grow(d_norms, sizeof(float) * (size_t)cap, sizeof(float) * (size_t)ntotal, s);
    norms_cap = cap;
  }

  // n rows (device-resident, or host rows when from_host) behind the image with their norms;
  // returns when they are in place
  void add_rows(int64_t n, const float* x, bool from_host, hipStream_t s) {
    reserve_rows(n, s);
    if (from_host) quiesce();
    else order_after(s);
    float* dst = base() + (size_t)ntotal * d;
    HIPCHECK(hipMemcpyAsync(dst, x, sizeof(float) * (size_t)n * d, from_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, s));
    launch_row_norms(dst, n, d, d_norms.as<float>() + ntotal, s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    ntotal += n;
    if (from_host) rows_from_host += n;
  }

  void reset_rows() {
    reset();
    d_norms.release();
    norms_cap = 0;
  }

  // n device-resident queries -> D, I (device), all on s
  void search_dev(int64_t n, const float* xd, int k, float* D, int64_t* I, hipStream_t s) {
    if (n == 0) return;
    order_after(s);
    if (ntotal == 0) {
      launch_fill_empty(D, I, n * k, ip(), s);
      HIPCHECK(hipGetLastError());
      mark_done(s);
      return;
    }
    FlatScanPlan pl;
    const int64_t qc = flat_query_chunk(n, ntotal, k, range_rows, &pl);
    w_xn.ensure(sizeof(float) * qc);
    p_tau.ensure(sizeof(uint32_t) * qc);
    p_partD.ensure(sizeof(float) * (size_t)pl.S * qc * k);
    p_partI.ensure(sizeof(int64_t) * (size_t)pl.S * qc * k);
    const size_t tmp_lists = (size_t)std::max(1, pl.S / pl.fan);
    p_tmpD.ensure(sizeof(float) * tmp_lists * qc * k);
    p_tmpI.ensure(sizeof(int64_t) * tmp_lists * qc * k);
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      const int64_t c = std::min(qc, n - q0);
      const float* xq = xd + q0 * d;
      launch_row_norms(xq, c, d, w_xn.as<float>(), s);
      FlatScanArgs a;
      a.x = xq;
      a.xn = w_xn.as<float>();
      a.nq = c;
      a.d = d;
      a.base = base();
      a.bn = d_norms.as<float>();
      a.nb = ntotal;
      a.k = k;
      a.ip = ip();
      a.tau = p_tau.as<uint32_t>();
      a.partD = p_partD.as<float>();
      a.partI = p_partI.as<int64_t>();
      a.tmpD = p_tmpD.as<float>();
      a.tmpI = p_tmpI.as<int64_t>();
      a.D = D + q0 * k;
      a.I = I + q0 * k;
      // (a shorter last chunk keeps the plan: its tile and ranges are valid for any nq)
      launch_flat_search(a, pl, s);
      HIPCHECK(hipGetLastError());
    }
    mark_done(s);
  }

  void search_host(int64_t n, const float* x, int k, float* D, int64_t* I) {
    if (n == 0) return;
    quiesce();
    w_x.ensure(sizeof(float) * n * d);
    w_D.ensure(sizeof(float) * n * k);
    w_I.ensure(sizeof(int64_t) * n * k);
    HIPCHECK(hipMemcpyAsync(w_x.p, x, sizeof(float) * n * d, hipMemcpyHostToDevice, stream));
    search_dev(n, w_x.as<float>(), k, w_D.as<float>(), w_I.as<int64_t>(), stream);
    HIPCHECK(hipMemcpyAsync(D, w_D.p, sizeof(float) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipMemcpyAsync(I, w_I.p, sizeof(int64_t) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
};

extern "C" {

int ivfpq_flat_index_create(int device, int d, int metric, ivfpq_flat_index** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    require(d >= 1, "IndexFlat: d must be at least 1 (d = " + std::to_string(d) + ")");
    require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT, "unknown metric");
    auto h = std::make_unique<ivfpq_flat_index>();
    h->d = d;
    h->metric = metric;
    h->row_bytes = sizeof(float) * (size_t)d;
    open_store(std::move(h), device, out);
  });
}

int ivfpq_flat_index_free(ivfpq_flat_index* h) { return free_handle(h); }

int ivfpq_flat_index_reset(ivfpq_flat_index* h) {
  return with_handle(h, [&] { h->reset_rows(); });
}

int ivfpq_flat_index_add(ivfpq_flat_index* h, int64_t n, const float* x) {
  return with_handle(h, [&] {
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_rows(n, x, true, h->stream);
  });
}

int ivfpq_flat_index_add_device(ivfpq_flat_index* h, int64_t n, const float* x, void* stream) {
  return with_handle(h, [&] {
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_rows(n, x, false, (hipStream_t)stream);
  });
}

// (the searches check their arguments before the handle)
int ivfpq_flat_index_search(ivfpq_flat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I) {
  return guarded([&] {
    check_flat_search_args(true, n, x, k, D, I);  // nothing to train
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->search_host(n, x, k, D, I);
  });
}

int ivfpq_flat_index_search_device(ivfpq_flat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I,
                                   void* stream) {
  return guarded([&] {
    check_flat_search_args(true, n, x, k, D, I);  // nothing to train
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->search_dev(n, x, k, D, I, (hipStream_t)stream);
  });
}

int64_t ivfpq_flat_index_ntotal(const ivfpq_flat_index* h) { return h ? h->ntotal : -1; }

int ivfpq_flat_index_get_dims(const ivfpq_flat_index* h, int* d, int* metric) {
  return guarded([&] {
    check_handle(h);
    if (d) *d = h->d;
    if (metric) *metric = h->metric;
  });
}

int ivfpq_flat_index_get_rows(ivfpq_flat_index* h, int64_t i0, int64_t n, float* out) {
  return with_handle(h, [&] {
    require(i0 >= 0 && n >= 0 && i0 + n <= h->ntotal, "row range outside [0, ntotal)");
    if (n == 0) return;
    require(out != nullptr, "null output pointer");
    h->read_rows(i0, n, reinterpret_cast<uint8_t*>(out), h->row_bytes);
  });
}

int ivfpq_flat_index_get_stats(ivfpq_flat_index* h, int64_t* rows_from_host, int64_t* capacity, int64_t* reallocs) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    if (rows_from_host) *rows_from_host = h->rows_from_host;
    if (capacity) *capacity = h->cap;
    if (reallocs) *reallocs = h->reallocs;
  });
}

int ivfpq_flat_index_set_range_rows(ivfpq_flat_index* h, int64_t rows) {
  return guarded([&] {
    check_handle(h);
    require(rows >= 0, "negative range size");
    std::lock_guard<std::mutex> lk(h->mu);
    h->range_rows = rows;
  });
}

int ivfpq_flat_index_get_plan(int64_t nq, int64_t nb, int k, int64_t set_rows, int* tile_q, int64_t* range_rows,
                              int* ranges, int* S, int* fan, int* rounds, int64_t* query_chunk) {
  return guarded([&] {
    require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
    require(nb >= 0 && nb < (int64_t)INT32_MAX && nq >= 0 && set_rows >= 0, "nb / nq / range size out of range");
    FlatScanPlan pl;
    const int64_t qc = flat_query_chunk(nq, nb, k, set_rows, &pl);
    if (tile_q) *tile_q = pl.tile_q;
    if (range_rows) *range_rows = pl.range_rows;
    if (ranges) *ranges = pl.ranges;
    if (S) *S = pl.S;
    if (fan) *fan = pl.fan;
    if (rounds) *rounds = pl.rounds;
    if (query_chunk) *query_chunk = qc;
  });
}

}  // extern "C"
