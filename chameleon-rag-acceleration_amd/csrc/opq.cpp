// The resident OPQ trainer (faiss_amd.OPQMatrix.train_device) behind the C-ABI of include/ivfpq.h.
// A handle keeps the centred training rows, their rotation, the PQ codes and the codebook in HBM
// across the outer rounds; one ivfpq_opq_iterate is one round up to the cross matrix
// C = xt^T rec, whose d x d2 SVD the caller takes on the host in float64.
// The Lloyd update is km_update.h's ordered fp64 accumulation over the [n M][dsub] view of the
// rotated rows: row r M + m belongs to cluster m 256 + code[r][m].
#include <atomic>
#include <vector>

#include "code_store.h"  // open_store
#include "ivfpq.h"
#include "km_update.h"
#include "opq_train.h"
#include "pca_moments.h"

using namespace chivf;

namespace {

std::atomic<int64_t> g_opq_chunk_rows{0};  // > 0: the cross's row chunk (ivfpq_opq_set_chunk_rows)

void check_opq_dims(int d, int d2, int M) {
  require(d >= 1 && d <= (1 << 16), "OPQ: d must be in [1, 65536] (d = " + std::to_string(d) + ")");
  require(M >= 1, "OPQ: M must be at least 1 (M = " + std::to_string(M) + ")");
  require(d2 >= 1 && d2 <= d, "OPQ: d2 must be in [1, d] (d2 = " + std::to_string(d2) + ", d = " + std::to_string(d) + ")");
  require(d2 % M == 0, "OPQ: d2 = " + std::to_string(d2) + " must be a multiple of M = " + std::to_string(M));
}

// the plan of the cross of ivfpq_opq_iterate, or the reason the shape cannot run
OpqPlan checked_opq_plan(int64_t n, int d, int d2) {
  require(n >= 1, "OPQ: need at least one row (n = " + std::to_string(n) + ")");
  require(d >= 1 && d <= (1 << 16) && d2 >= 1 && d2 <= d, "OPQ: need 1 <= d2 <= d <= 65536");
  const OpqPlan p = opq_plan(n, d, d2, g_opq_chunk_rows.load());
  require(p.chunks <= kOpqMaxChunks && (int64_t)p.chunks * p.tiles < (int64_t)INT32_MAX / 16,
          "too many row chunks for one launch: raise the chunk length");
  return p;
}

}  // namespace

struct ivfpq_opq : StreamOrder {
  int device = 0, d = 0, d2 = 0, M = 0;
  int64_t n = 0;  // rows held (0: none yet)
  bool have_cb = false;
  bool have_codes = false;  // d_codes holds the final assignment of an iterate over the rows held
  hipStream_t stream = nullptr;
  std::mutex mu;
  DevBuf d_raw, d_psum, d_mean, d_xt, d_xp, d_codes, d_labels, d_zero, d_cb, d_sum, d_cnt, d_obj, d_pass, d_AT, d_idx,
      d_part, d_cross;
  KmPassScratch w;

  ~ivfpq_opq() {
    if (stream) (void)hipStreamDestroy(stream);
  }
  int dsub() const { return d2 / M; }
  int ncent() const { return M * 256; }

  void ensure_codebook() {
    d_cb.ensure(sizeof(float) * (size_t)ncent() * dsub());
    d_sum.ensure(sizeof(double) * (size_t)ncent() * dsub());
    d_cnt.ensure(sizeof(int64_t) * (size_t)ncent());
  }

  // x: n_ rows in HBM, ready on s; centres them into d_xt and sizes everything that depends on n
  void take_rows(int64_t n_, const float* x, hipStream_t s) {
    require(n_ >= 1, "OPQ: need at least one row (n = " + std::to_string(n_) + ")");
    require(n_ * M < (int64_t)INT32_MAX, "OPQ: n M must stay below 2^31 - 1");
    (void)checked_opq_plan(n_, d, d2);
    const size_t nm = (size_t)n_ * M;
    have_codes = false;
    d_psum.ensure(sizeof(double) * (size_t)pca_mean_chunks(n_) * d);
    d_mean.ensure(sizeof(float) * (size_t)d);
    d_xt.ensure(sizeof(float) * (size_t)n_ * d);
    d_xp.ensure(sizeof(float) * (size_t)n_ * d2);
    d_codes.ensure(nm);
    d_labels.ensure(sizeof(int64_t) * nm);
    d_zero.ensure(sizeof(float) * nm);
    d_obj.ensure(sizeof(double));
    d_pass.ensure(km_pass_scratch_bytes((int64_t)nm, ncent(), 0));
    w = km_pass_scratch(d_pass.p, (int64_t)nm, ncent(), 0);
    ensure_codebook();
    launch_pca_mean(x, n_, d, d_psum.as<double>(), d_mean.as<float>(), s);
    launch_opq_center(x, n_, d, d_mean.as<float>(), d_xt.as<float>(), s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemsetAsync(d_zero.p, 0, sizeof(float) * nm, s));  // launch_km_pass's keys: its objective is unused
    HIPCHECK(hipMemsetAsync(d_obj.p, 0, sizeof(double), s));
    HIPCHECK(hipStreamSynchronize(s));
    n = n_;
  }

  void iterate(const float* A, int niter_pq, const int64_t* init_rows, float* cross) {
    require(n > 0, "OPQ: no training rows (ivfpq_opq_set_rows first)");
    require(A != nullptr && cross != nullptr, "null A / cross");
    require(niter_pq >= 0, "OPQ: niter_pq must be at least 0 (niter_pq = " + std::to_string(niter_pq) + ")");
    require(have_cb || init_rows != nullptr, "OPQ: no codebook (ivfpq_opq_set_codebook, or pass init_rows)");
    const OpqPlan pl = checked_opq_plan(n, d, d2);
    const hipStream_t s = stream;
    const int ds = dsub(), k = ncent();
    const int64_t nm = n * M;
    std::vector<int64_t> idx;
    if (init_rows) {  // centroid (m, j) starts at sub-vector m of row init_rows[m 256 + j]
      idx.resize((size_t)k);
      for (int c = 0; c < k; c++) {
        require(init_rows[c] >= 0 && init_rows[c] < n, "OPQ: init_rows[" + std::to_string(c) + "] is outside [0, n)");
        idx[c] = init_rows[c] * M + c / 256;
      }
    }
    std::vector<float> AT((size_t)d * d2);
    for (int j = 0; j < d2; j++)
      for (int t = 0; t < d; t++) AT[(size_t)t * d2 + j] = A[(size_t)j * d + t];
    d_AT.ensure(sizeof(float) * AT.size());
    d_part.ensure(opq_cross_workspace_bytes(pl));
    d_cross.ensure(sizeof(float) * (size_t)d * d2);
    HIPCHECK(hipMemcpyAsync(d_AT.p, AT.data(), sizeof(float) * AT.size(), hipMemcpyHostToDevice, s));
    if (init_rows) {
      d_idx.ensure(sizeof(int64_t) * (size_t)k);
      HIPCHECK(hipMemcpyAsync(d_idx.p, idx.data(), sizeof(int64_t) * (size_t)k, hipMemcpyHostToDevice, s));
    }
    HIPCHECK(hipStreamSynchronize(s));  // (AT and idx are read until here)
    launch_linear_transform(d_xt.as<float>(), n, d, d_AT.as<float>(), nullptr, d2, d_xp.as<float>(), s);
    if (init_rows) {
      launch_km_gather_rows(d_xp.as<float>(), ds, d_idx.as<int64_t>(), k, d_cb.as<float>(), s);
      have_cb = true;
    }
    HIPCHECK(hipGetLastError());
    for (int it = 0; it < niter_pq; it++) {
      launch_opq_assign(d_xp.as<float>(), n, d2, d_cb.as<float>(), M, d_codes.as<uint8_t>(), s);
      launch_opq_labels(d_codes.as<uint8_t>(), n, M, d_labels.as<int64_t>(), s);
      HIPCHECK(hipMemsetAsync(d_sum.p, 0, sizeof(double) * (size_t)k * ds, s));
      HIPCHECK(hipMemsetAsync(d_cnt.p, 0, sizeof(int64_t) * (size_t)k, s));
      HIPCHECK(launch_km_pass(d_xp.as<float>(), nm, ds, k, d_labels.as<int64_t>(), d_zero.as<float>(), w,
                              d_sum.as<double>(), d_cnt.as<int64_t>(), d_obj.as<double>(), s));
      launch_km_mean(d_sum.as<double>(), d_cnt.as<int64_t>(), k, ds, d_cb.as<float>(), s);  // empty clusters stay
      HIPCHECK(hipGetLastError());
    }
    launch_opq_assign(d_xp.as<float>(), n, d2, d_cb.as<float>(), M, d_codes.as<uint8_t>(), s);
    launch_opq_cross(d_xt.as<float>(), n, d, d_codes.as<uint8_t>(), d_cb.as<float>(), d2, M, pl, d_part.as<float>(),
                     d_cross.as<float>(), s);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(cross, d_cross.p, sizeof(float) * (size_t)d * d2, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    have_codes = true;
  }
};

extern "C" {

int ivfpq_opq_create(int d, int d2, int M, int device, ivfpq_opq** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    check_opq_dims(d, d2, M);
    auto h = std::make_unique<ivfpq_opq>();
    h->d = d;
    h->d2 = d2;
    h->M = M;
    open_store(std::move(h), device, out);
  });
}

int ivfpq_opq_free(ivfpq_opq* h) { return free_handle(h); }

int ivfpq_opq_set_rows(ivfpq_opq* h, int64_t n, const float* x) {
  return with_handle(h, [&] {
    require(x != nullptr && n >= 1, "empty training set");
    h->d_raw.ensure(sizeof(float) * (size_t)n * h->d);
    HIPCHECK(hipMemcpyAsync(h->d_raw.p, x, sizeof(float) * (size_t)n * h->d, hipMemcpyHostToDevice, h->stream));
    h->take_rows(n, h->d_raw.as<float>(), h->stream);
    h->d_raw.release();
  });
}

int ivfpq_opq_set_rows_device(ivfpq_opq* h, int64_t n, const float* x, void* stream) {
  return with_handle(h, [&] {
    require(x != nullptr && n >= 1, "empty training set");
    h->take_rows(n, x, (hipStream_t)stream);
  });
}

int ivfpq_opq_set_codebook(ivfpq_opq* h, const float* cb) {
  return with_handle(h, [&] {
    require(cb != nullptr, "null codebook");
    h->ensure_codebook();
    const size_t bytes = sizeof(float) * (size_t)h->ncent() * h->dsub();
    HIPCHECK(hipMemcpyAsync(h->d_cb.p, cb, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->have_cb = true;
  });
}

int ivfpq_opq_get_codebook(ivfpq_opq* h, float* cb) {
  return with_handle(h, [&] {
    require(cb != nullptr, "null output pointer");
    require(h->have_cb, "OPQ: no codebook yet");
    const size_t bytes = sizeof(float) * (size_t)h->ncent() * h->dsub();
    HIPCHECK(hipMemcpyAsync(cb, h->d_cb.p, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  });
}

int ivfpq_opq_get_codes(ivfpq_opq* h, uint8_t* codes) {
  return with_handle(h, [&] {
    require(codes != nullptr, "null output pointer");
    require(h->have_codes, "OPQ: no codes yet (ivfpq_opq_iterate first)");
    HIPCHECK(hipMemcpyAsync(codes, h->d_codes.p, (size_t)h->n * h->M, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  });
}

int ivfpq_opq_iterate(ivfpq_opq* h, const float* A, int niter_pq, const int64_t* init_rows, float* cross) {
  return with_handle(h, [&] { h->iterate(A, niter_pq, init_rows, cross); });
}

int ivfpq_opq_set_chunk_rows(int64_t rows) {
  return guarded([&] {
    require(rows >= 0, "negative chunk length");
    g_opq_chunk_rows.store(rows);
  });
}

int ivfpq_opq_get_plan(int64_t n, int d, int d2, int* chunks, int64_t* chunk_rows, int* tiles) {
  return guarded([&] {
    const OpqPlan p = checked_opq_plan(n, d, d2);
    if (chunks) *chunks = p.chunks;
    if (chunk_rows) *chunk_rows = p.chunk_rows;
    if (tiles) *tiles = p.tiles;
  });
}

}  // extern "C"
