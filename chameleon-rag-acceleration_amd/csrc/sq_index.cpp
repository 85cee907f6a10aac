// Flat scalar quantizer (IndexScalarQuantizer) behind the C-ABI of include/ivfpq.h.
// faiss.IndexScalarQuantizer: every component stored as a half or as an 8-bit code
// between the trained per-dimension (or global) minimum and maximum, every code scanned
// for every query with the decode fused in (sq_scan.hip).  The codes live in a CodeStore
// of code_size bytes per row, with the scan's read slack behind the image.
#include <cstring>
#include <vector>

#include "code_store.h"
#include "ivfpq.h"
#include "sq_params.h"
#include "sq_scan.h"

using namespace chivf;

struct ivfpq_sq_index : CodeStore {
  int d = 0, qtype = IVFPQ_SQ_FP16, metric = IVFPQ_METRIC_L2;
  int codec = SQ_CODEC_FP16, code_size = 0;
  bool trained = false;
  std::vector<float> params;  // Faiss's sq.trained: [vmin (d), vdiff (d)], [vmin, vdiff] (uniform) or empty (fp16)
  DevBuf d_vmin, d_vdiff;
  DevBuf w_codes, w_mm, w_D, w_I, p_tau, p_partD, p_partI, p_tmpD, p_tmpI;

  ivfpq_sq_index() : CodeStore("IndexScalarQuantizer") {}
  bool ip() const { return metric == IVFPQ_METRIC_INNER_PRODUCT; }
  bool uniform() const { return qtype == IVFPQ_SQ_8BIT_UNIFORM; }
  size_t nparams() const { return sq_nparams(qtype, d); }
  int64_t host_rows(int64_t n) const { return CodeStore::host_rows(n, sizeof(float) * d); }

  // the 8-bit codec's device parameters: per dimension, a uniform pair repeated d times
  void upload_params() {
    quiesce();
    if (codec == SQ_CODEC_8BIT) sq_upload_params(params, qtype, d, d_vmin, d_vdiff, stream);
    trained = true;
  }

  // RS_minmax with rangestat_arg = 0 over n host vectors
  void train_host(int64_t n, const float* x) {
    if (codec == SQ_CODEC_FP16) return;
    quiesce();
    const int64_t rows = host_rows(n);
    w_x.ensure(sizeof(float) * rows * d);
    w_mm.ensure(sizeof(uint32_t) * 2 * d);
    uint32_t* lo = w_mm.as<uint32_t>();
    uint32_t* hi = lo + d;
    launch_sq_minmax_init(lo, hi, d, stream);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      HIPCHECK(hipMemcpyAsync(w_x.p, x + r0 * d, sizeof(float) * c * d, hipMemcpyHostToDevice, stream));
      launch_sq_minmax(w_x.as<float>(), c, d, lo, hi, stream);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipStreamSynchronize(stream));  // w_x is reused
    }
    std::vector<uint32_t> bits(2 * (size_t)d);
    HIPCHECK(hipMemcpyAsync(bits.data(), w_mm.p, sizeof(uint32_t) * 2 * d, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    params = sq_trained_from_minmax(bits, qtype, d);
    upload_params();
  }

  // encode n device-resident vectors behind the image; returns when they are in place
  void add_dev(int64_t n, const float* xd, hipStream_t s) {
    reserve(n, s);
    order_after(s);
    launch_sq_encode(codec, xd, n, d, d_vmin.as<float>(), d_vdiff.as<float>(), row(ntotal), s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    ntotal += n;
  }

  // sa_encode / sa_decode of host buffers, in chunks through the staging buffers
  void encode_host(int64_t n, const float* x, uint8_t* out) {
    const int64_t rows = host_rows(n);
    quiesce();
    w_x.ensure(sizeof(float) * rows * d);
    w_codes.ensure((size_t)rows * code_size);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      HIPCHECK(hipMemcpyAsync(w_x.p, x + r0 * d, sizeof(float) * c * d, hipMemcpyHostToDevice, stream));
      launch_sq_encode(codec, w_x.as<float>(), c, d, d_vmin.as<float>(), d_vdiff.as<float>(), w_codes.as<uint8_t>(),
                       stream);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipMemcpyAsync(out + r0 * code_size, w_codes.p, (size_t)c * code_size, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipStreamSynchronize(stream));
    }
  }
  void decode_host(int64_t n, const uint8_t* codes, float* out) {
    const int64_t rows = host_rows(n);
    quiesce();
    w_x.ensure(sizeof(float) * rows * d);
    w_codes.ensure((size_t)rows * code_size);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      HIPCHECK(hipMemcpyAsync(w_codes.p, codes + r0 * code_size, (size_t)c * code_size, hipMemcpyHostToDevice, stream));
      launch_sq_decode(codec, w_codes.as<uint8_t>(), c, d, d_vmin.as<float>(), d_vdiff.as<float>(), w_x.as<float>(),
                       stream);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipMemcpyAsync(out + r0 * d, w_x.p, sizeof(float) * c * d, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipStreamSynchronize(stream));
    }
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
    const IvfFlatPlan pl = ivfflat_plan(k, sq_scan_ranges(ntotal));
    const int64_t qc = partial_query_chunk(n, pl.S, k);
    p_tau.ensure(sizeof(uint32_t) * qc);
    p_partD.ensure(sizeof(float) * (size_t)pl.S * qc * k);
    p_partI.ensure(sizeof(int64_t) * (size_t)pl.S * qc * k);
    const size_t tmp_lists = (size_t)std::max(1, pl.S / pl.fan);
    p_tmpD.ensure(sizeof(float) * tmp_lists * qc * k);
    p_tmpI.ensure(sizeof(int64_t) * tmp_lists * qc * k);
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      SqScanArgs a;
      a.codec = codec;
      a.x = xd + q0 * d;
      a.nq = std::min(qc, n - q0);
      a.d = d;
      a.codes = d_codes.as<uint8_t>();
      a.nb = ntotal;
      a.vmin = d_vmin.as<float>();
      a.vdiff = d_vdiff.as<float>();
      a.k = k;
      a.ip = ip();
      a.tau = p_tau.as<uint32_t>();
      a.partD = p_partD.as<float>();
      a.partI = p_partI.as<int64_t>();
      a.tmpD = p_tmpD.as<float>();
      a.tmpI = p_tmpI.as<int64_t>();
      a.D = D + q0 * k;
      a.I = I + q0 * k;
      launch_sq_search(a, pl, s);
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

int ivfpq_sq_create(int d, int qtype, int metric, int device, ivfpq_sq_index** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    require(d >= 4 && d <= 2048 && d % 4 == 0,
            "IndexScalarQuantizer: d must be a multiple of 4 in [4, 2048] (d = " + std::to_string(d) + ")");
    check_sq_qtype(qtype);
    require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT, "unknown metric");
    auto h = std::make_unique<ivfpq_sq_index>();
    h->d = d;
    h->qtype = qtype;
    h->codec = sq_codec_of(qtype);
    h->code_size = sq_code_size(h->codec, d);
    h->row_bytes = (size_t)h->code_size;
    h->slack = kSqScanSlack;  // the scan's 16-byte loads may straddle the last row's end
    h->metric = metric;
    h->trained = qtype == IVFPQ_SQ_FP16;  // nothing to train
    open_store(std::move(h), device, out);
  });
}

int ivfpq_sq_free(ivfpq_sq_index* h) { return free_handle(h); }

int ivfpq_sq_train(ivfpq_sq_index* h, int64_t n, const float* x) {
  return with_handle(h, [&] {
    require(x != nullptr && n > 0, "empty training set");
    h->train_host(n, x);
  });
}

int ivfpq_sq_set_trained(ivfpq_sq_index* h, const float* trained, int64_t count) {
  return with_handle(h, [&] {
    require(count == (int64_t)h->nparams(),
            "trained has " + std::to_string(count) + " values, this quantizer " + std::to_string(h->nparams()));
    require(count == 0 || trained != nullptr, "null trained");
    h->params.assign(trained, trained + count);
    h->upload_params();
  });
}

int ivfpq_sq_add(ivfpq_sq_index* h, int64_t n, const float* x) {
  return with_handle(h, [&] {
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_host(n, x, sizeof(float) * h->d, [&](int64_t c) { h->add_dev(c, h->w_x.as<float>(), h->stream); });
  });
}

int ivfpq_sq_add_device(ivfpq_sq_index* h, int64_t n, const float* x, void* stream) {
  return with_handle(h, [&] {
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, (hipStream_t)stream);
  });
}

int ivfpq_sq_add_codes(ivfpq_sq_index* h, int64_t n, const uint8_t* codes) {
  return with_handle(h, [&] {
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(codes != nullptr, "null codes");
    h->append_rows(n, codes);
  });
}

int ivfpq_sq_reset(ivfpq_sq_index* h) {
  return with_handle(h, [&] { h->reset(); });
}

int ivfpq_sq_search(ivfpq_sq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I) {
  return with_handle(h, [&] {
    check_flat_search_args(h->trained, n, x, k, D, I);
    h->search_host(n, x, k, D, I);
  });
}

int ivfpq_sq_search_device(ivfpq_sq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I, void* stream) {
  return with_handle(h, [&] {
    check_flat_search_args(h->trained, n, x, k, D, I);
    h->search_dev(n, x, k, D, I, (hipStream_t)stream);
  });
}

int64_t ivfpq_sq_ntotal(const ivfpq_sq_index* h) { return h ? h->ntotal : -1; }

int ivfpq_sq_is_trained(const ivfpq_sq_index* h) { return h && h->trained ? 1 : 0; }

int ivfpq_sq_get_dims(const ivfpq_sq_index* h, int* d, int* qtype, int* metric, int* code_size) {
  return guarded([&] {
    check_handle(h);
    if (d) *d = h->d;
    if (qtype) *qtype = h->qtype;
    if (metric) *metric = h->metric;
    if (code_size) *code_size = h->code_size;
  });
}

int ivfpq_sq_get_trained(const ivfpq_sq_index* h, float* out, int64_t* count) {
  return guarded([&] {
    check_handle(h);
    require(h->trained, "index is not trained");
    if (count) *count = (int64_t)h->params.size();
    if (out && !h->params.empty()) std::memcpy(out, h->params.data(), sizeof(float) * h->params.size());
  });
}

int ivfpq_sq_get_codes(ivfpq_sq_index* h, int64_t i0, int64_t n, uint8_t* out) {
  return with_handle(h, [&] {
    require(i0 >= 0 && n >= 0 && i0 + n <= h->ntotal, "code range outside [0, ntotal)");
    if (n == 0) return;
    require(out != nullptr, "null output pointer");
    h->read_rows(i0, n, out, h->row_bytes);
  });
}

int ivfpq_sq_encode(ivfpq_sq_index* h, int64_t n, const float* x, uint8_t* codes) {
  return with_handle(h, [&] {
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr && codes != nullptr, "null x / codes");
    h->encode_host(n, x, codes);
  });
}

int ivfpq_sq_decode(ivfpq_sq_index* h, int64_t n, const uint8_t* codes, float* x) {
  return with_handle(h, [&] {
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr && codes != nullptr, "null x / codes");
    h->decode_host(n, codes, x);
  });
}

// ---- how the batches are cut: host arithmetic, no handle ----
int ivfpq_sq_get_plan(int64_t nq, int64_t nb, int k, int* S, int* fan, int64_t* query_chunk) {
  return guarded([&] {
    require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
    require(nb >= 0 && nb < (int64_t)INT32_MAX && nq >= 0, "nb / nq out of range");
    const IvfFlatPlan pl = ivfflat_plan(k, sq_scan_ranges(nb));
    if (S) *S = pl.S;
    if (fan) *fan = pl.fan;
    if (query_chunk) *query_chunk = partial_query_chunk(nq, pl.S, k);
  });
}

int ivfpq_host_get_pass_rows(int64_t n, int64_t in_bytes, int64_t* rows) {
  return guarded([&] {
    require(n >= 0 && in_bytes >= 1, "shape out of range");
    if (rows) *rows = CodeStore::host_rows(n, (size_t)in_bytes);
  });
}

}  // extern "C"
