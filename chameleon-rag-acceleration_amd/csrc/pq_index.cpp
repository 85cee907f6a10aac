// Flat PQ (IndexPQ) behind the C-ABI of include/ivfpq.h.
// faiss.IndexPQ: no coarse quantizer and no inverted lists -- one product quantizer
// over the raw vectors, every code scanned for every query (pq_flat.hip).  The codes
// live in a CodeStore of M bytes per row.
#include <cstring>
#include <vector>

#include "code_store.h"
#include "ivf_flat.h"  // launch_fill_empty
#include "ivfpq.h"
#include "ivfpq_test.h"
#include "kmeans.h"
#include "pq_flat.h"

using namespace chivf;

namespace {

// queries per chunk of a flat-PQ search: the tables (M KiB per query) within kChunkBytes,
// the grid's y extent (shared by the handle and ivfpq_pq_debug_plan)
int64_t pq_query_chunk(int M, int64_t n) {
  return std::max<int64_t>(1, std::min<int64_t>({n, (int64_t)(kChunkBytes / ((size_t)M * 1024)), 4096}));
}

const char* pq_supported_M_text() { return " not supported on the GPU (8, 16, 32, 48, 64, 80, 96, 112, 128)"; }

}  // namespace

struct ivfpq_pq_index : CodeStore {
  int d = 0, M = 0, nbits = 8, ksub = 256, metric = IVFPQ_METRIC_L2;
  bool trained = false;
  std::vector<float> codebook;  // [M][256][d / M]
  DevBuf d_cb;
  DevBuf w_tab, w_pD, w_pI, w_D, w_I;  // tables, partial lists, results of the host entry points

  ivfpq_pq_index() : CodeStore("IndexPQ") {}
  bool ip() const { return metric == IVFPQ_METRIC_INNER_PRODUCT; }

  void upload_codebook() {
    quiesce();
    d_cb.ensure(sizeof(float) * codebook.size());
    HIPCHECK(hipMemcpyAsync(d_cb.p, codebook.data(), sizeof(float) * codebook.size(), hipMemcpyHostToDevice, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    trained = true;
  }

  // encode n device-resident vectors behind the image; returns when they are in place
  void add_dev(int64_t n, const float* xd, hipStream_t s) {
    reserve(n, s);
    order_after(s);
    launch_pq_encode_flat(xd, n, d, d_cb.as<float>(), M, row(ntotal), s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    ntotal += n;
  }

  int64_t query_chunk(int64_t n) const { return pq_query_chunk(M, n); }

  // c device-resident queries -> D, I (device), all on s
  void search_chunk(const float* xd, int64_t c, int k, float* D, int64_t* I, hipStream_t s) {
    if (ntotal == 0) {
      launch_fill_empty(D, I, c * k, ip(), s);
      return;
    }
    w_tab.ensure(sizeof(float) * c * M * 256);
    if (ip())
      launch_ip_table(xd, c, d, d_cb.as<float>(), M, ksub, w_tab.as<float>(), s);
    else
      launch_l2_table(xd, c, d, d_cb.as<float>(), M, w_tab.as<float>(), s);
    const PqScanPlan pl = pq_scan_plan(M, k, c, ntotal);
    w_pD.ensure(sizeof(float) * pl.S * c * k);
    w_pI.ensure(sizeof(int64_t) * pl.S * c * k);
    launch_pq_scan(w_tab.as<float>(), c, d_codes.as<uint8_t>(), ntotal, M, k, ip(), pl, w_pD.as<float>(),
                   w_pI.as<int64_t>(), s);
    launch_merge_topk(pl.S, c, k, w_pD.as<float>(), w_pI.as<int64_t>(), D, I, s, ip());
    HIPCHECK(hipGetLastError());
  }

  void search_dev(int64_t n, const float* xd, int k, float* D, int64_t* I, hipStream_t s) {
    const int64_t qc = query_chunk(n);
    order_after(s);
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      const int64_t c = std::min(qc, n - q0);
      search_chunk(xd + q0 * d, c, k, D + q0 * k, I + q0 * k, s);
    }
    mark_done(s);
  }

  void search_host(int64_t n, const float* x, int k, float* D, int64_t* I) {
    const int64_t qc = query_chunk(n);
    quiesce();
    w_x.ensure(sizeof(float) * qc * d);
    w_D.ensure(sizeof(float) * qc * k);
    w_I.ensure(sizeof(int64_t) * qc * k);
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      const int64_t c = std::min(qc, n - q0);
      HIPCHECK(hipMemcpyAsync(w_x.p, x + q0 * d, sizeof(float) * c * d, hipMemcpyHostToDevice, stream));
      search_chunk(w_x.as<float>(), c, k, w_D.as<float>(), w_I.as<int64_t>(), stream);
      HIPCHECK(hipMemcpyAsync(D + q0 * k, w_D.p, sizeof(float) * c * k, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipMemcpyAsync(I + q0 * k, w_I.p, sizeof(int64_t) * c * k, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipStreamSynchronize(stream));
    }
  }
};

extern "C" {

int ivfpq_pq_create(int d, int M, int nbits, int metric, int device, ivfpq_pq_index** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    require(d > 0 && M > 0, "d and M must be positive");
    require(d % M == 0, "d must be a multiple of M");
    require(nbits == 8, "only nbits=8 is supported");
    require(pq_flat_supported_M(M), "M=" + std::to_string(M) + pq_supported_M_text());
    require(d <= 2048, "d > 2048 not supported");
    require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT, "unknown metric");
    auto h = std::make_unique<ivfpq_pq_index>();
    h->d = d;
    h->M = M;
    h->nbits = nbits;
    h->metric = metric;
    h->row_bytes = (size_t)M;
    open_store(std::move(h), device, out);
  });
}

int ivfpq_pq_free(ivfpq_pq_index* h) { return free_handle(h); }

int ivfpq_pq_train(ivfpq_pq_index* h, int64_t n, const float* x, int niter, uint64_t seed) {
  return with_handle(h, [&] {
    require(x != nullptr && n > 0, "empty training set");
    const int d = h->d, M = h->M, dsub = d / M;
    // the k-means of ivfpq_train's sub-quantizers (assignment on the GPU, double-precision
    // mean on the host), on the handle's stream
    KMeans km(h->stream);
    std::vector<float> sub((size_t)n * dsub);
    std::vector<float> cb((size_t)M * 256 * dsub);
    for (int m = 0; m < M; m++) {
      for (int64_t i = 0; i < n; i++) std::memcpy(&sub[(size_t)i * dsub], x + i * d + m * dsub, sizeof(float) * dsub);
      km.kmeans(sub.data(), n, dsub, 256, niter, seed + 1 + (uint64_t)m, cb.data() + (size_t)m * 256 * dsub);
    }
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->codebook = std::move(cb);
    h->upload_codebook();
  });
}

int ivfpq_pq_set_trained(ivfpq_pq_index* h, const float* codebook) {
  return with_handle(h, [&] {
    require(codebook != nullptr, "null codebook");
    h->codebook.assign(codebook, codebook + (size_t)h->M * 256 * (h->d / h->M));
    h->upload_codebook();
  });
}

int ivfpq_pq_add(ivfpq_pq_index* h, int64_t n, const float* x) {
  return with_handle(h, [&] {
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_host(n, x, sizeof(float) * h->d, [&](int64_t c) { h->add_dev(c, h->w_x.as<float>(), h->stream); });
  });
}

int ivfpq_pq_add_device(ivfpq_pq_index* h, int64_t n, const float* x, void* stream) {
  return with_handle(h, [&] {
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, (hipStream_t)stream);
  });
}

int ivfpq_pq_add_codes(ivfpq_pq_index* h, int64_t n, const uint8_t* codes) {
  return with_handle(h, [&] {
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(codes != nullptr, "null codes");
    h->append_rows(n, codes);
  });
}

int ivfpq_pq_reset(ivfpq_pq_index* h) {
  return with_handle(h, [&] { h->reset(); });
}

int ivfpq_pq_search(ivfpq_pq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I) {
  return with_handle(h, [&] {
    check_flat_search_args(h->trained, n, x, k, D, I);
    if (n == 0) return;
    h->search_host(n, x, k, D, I);
  });
}

int ivfpq_pq_search_device(ivfpq_pq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I, void* stream) {
  return with_handle(h, [&] {
    check_flat_search_args(h->trained, n, x, k, D, I);
    if (n == 0) return;
    h->search_dev(n, x, k, D, I, (hipStream_t)stream);
  });
}

int64_t ivfpq_pq_ntotal(const ivfpq_pq_index* h) { return h ? h->ntotal : -1; }

int ivfpq_pq_is_trained(const ivfpq_pq_index* h) { return h && h->trained ? 1 : 0; }

int ivfpq_pq_get_dims(const ivfpq_pq_index* h, int* d, int* M, int* nbits, int* metric) {
  return guarded([&] {
    check_handle(h);
    if (d) *d = h->d;
    if (M) *M = h->M;
    if (nbits) *nbits = h->nbits;
    if (metric) *metric = h->metric;
  });
}

int ivfpq_pq_get_codebook(const ivfpq_pq_index* h, float* out) {
  return guarded([&] {
    check_handle(h);
    require(h->trained, "index is not trained");
    require(out != nullptr, "null output pointer");
    std::memcpy(out, h->codebook.data(), sizeof(float) * h->codebook.size());
  });
}

int ivfpq_pq_get_codes(ivfpq_pq_index* h, int64_t i0, int64_t n, uint8_t* out) {
  return with_handle(h, [&] {
    require(i0 >= 0 && n >= 0 && i0 + n <= h->ntotal, "code range outside [0, ntotal)");
    if (n == 0) return;
    require(out != nullptr, "null output pointer");
    h->read_rows(i0, n, out, h->row_bytes);
  });
}

// Test hook (ivfpq_test.h): host arithmetic only, no handle and no device call.
int ivfpq_pq_debug_plan(int M, int k, int64_t nq, int64_t nb, int* G, int* ranges, int64_t* rows, int* S,
                        int64_t* query_chunk) {
  return guarded([&] {
    require(pq_flat_supported_M(M), "M=" + std::to_string(M) + pq_supported_M_text());
    require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
    require(nq >= 1, "query count must be positive");
    require(nb >= 1 && nb < (int64_t)INT32_MAX, "IndexPQ holds at most 2^31 - 2 codes");
    const int64_t qc = pq_query_chunk(M, nq);
    const PqScanPlan pl = pq_scan_plan(M, k, std::min(nq, qc), nb);
    if (G) *G = pl.G;
    if (ranges) *ranges = pl.ranges;
    if (rows) *rows = pl.rows;
    if (S) *S = pl.S;
    if (query_chunk) *query_chunk = qc;
  });
}

}  // extern "C"
