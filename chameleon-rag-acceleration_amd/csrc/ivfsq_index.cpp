// IVF over scalar-quantizer codes (IndexIVFScalarQuantizer) behind the C-ABI of include/ivfpq.h.
// faiss.IndexIVFScalarQuantizer: IVF-Flat's coarse quantizer, device list image and pending-add
// merge with the rows stored as the flat scalar quantizer's fp16 / 8-bit codes (sq_index.cpp),
// of the vector or, by_residual, of the vector minus its list's centroid; scanned by
// ivf_sq.hip.  The codes live only in the device image {list_off, codes, ids}, every list
// sorted by label, with the scan's read slack behind the last row; adds are encoded straight
// into a pending set on the device and merged with the image kernels of ivfpq_build.h at code
// size d or 2 d.  The handle -- image, pending set, workspaces, the search around the scan and
// the entry points that IVF-Flat has too -- is ivf_lists.h's IvfLists; this file keeps the
// codes: the quantizer's table and its training, the encoding adds, the by_residual
// workspaces, the scan's launch, create and the entry points' names.
#include <cstring>
#include <memory>
#include <vector>

#include "ivf_lists.h"
#include "ivf_sq.h"
#include "ivfpq.h"
#include "kmeans.h"
#include "sq_params.h"

using namespace chivf;

namespace {
constexpr int64_t kSqTrainRows = 100000;  // ScalarQuantizer::train_residual's subsample
constexpr uint64_t kSqTrainSeed = 1234;   // ... and its rand_perm seed
}  // namespace

struct ivfpq_ivfsq_index : IvfLists {
  int qtype = IVFPQ_SQ_FP16;
  int codec = SQ_CODEC_FP16, code_size = 0;
  bool by_residual = true;
  bool sq_trained = false;
  std::vector<float> params;  // Faiss's sq.trained
  DevBuf d_vmin, d_vdiff;
  DevBuf w_xa, w_mm;               // add / train staging
  DevBuf w_cd, p_probe, p_qr;      // by_residual: zero coarse values, probe columns, residual queries

  bool trained() const override { return cent_trained && sq_trained; }
  bool resid_q() const { return by_residual && !ip(); }     // residual queries
  bool coarse_add() const { return by_residual && ip(); }   // the pair's coarse value added

  IvfFlatPlan plan(int k, int64_t slots) const override { return ivfsq_plan(codec, k, slots); }
  // the probe column of every bucket entry beside the coarse keys and buckets
  size_t entry_bytes() const override { return by_residual ? 12 : 8; }
  bool resid_queries() const override { return resid_q(); }
  void prepare_chunks(int64_t qc, int np, bool zero_coarse, hipStream_t s) override {
    if (coarse_add() && zero_coarse) {
      w_cd.ensure(sizeof(float) * qc * np);
      HIPCHECK(hipMemsetAsync(w_cd.p, 0, sizeof(float) * qc * np, s));
    }
    if (by_residual) p_probe.ensure(sizeof(int32_t) * (size_t)nlist * qc);
    if (resid_q()) p_qr.ensure(sizeof(float) * (size_t)qc * np * d);
  }
  void launch_chunk(const IvfFlatArgs& f, const IvfFlatPlan& pl, const float* cdis, hipStream_t s) override {
    IvfSqArgs a;
    a.f = f;
    a.cdis = coarse_add() ? (cdis ? cdis : w_cd.as<float>()) : nullptr;
    a.codec = codec;
    a.codes = img.rows.as<uint8_t>();
    a.vmin = d_vmin.as<float>();
    a.vdiff = d_vdiff.as<float>();
    a.by_residual = by_residual;
    a.cent = cq.d_cent.as<float>();
    a.probe_of = p_probe.as<int32_t>();
    a.qr = p_qr.as<float>();
    launch_ivfsq_search(a, pl, s);
  }

  void upload_params() {
    quiesce();
    if (codec == SQ_CODEC_8BIT) sq_upload_params(params, qtype, d, d_vmin, d_vdiff, stream);
    sq_trained = true;
  }

  // The scalar quantizer's table: RS_minmax (rangestat_arg 0) over the first kSqTrainRows rows of
  // Faiss's rand_perm(n, 1234) (all rows when n is no larger), replaced by their residuals to
  // the coarse top-1 centroid when by_residual.
  void train_sq(int64_t n, const float* x) {
    if (codec == SQ_CODEC_FP16) {
      upload_params();
      return;
    }
    quiesce();
    std::vector<int64_t> pick;
    if (n > kSqTrainRows) pick = rand_perm_prefix(n, kSqTrainRows, kSqTrainSeed);
    const int64_t m = pick.empty() ? n : (int64_t)pick.size();
    const int64_t rows = chunk_rows(m, true);
    w_xa.ensure(sizeof(float) * rows * d);
    w_mm.ensure(sizeof(uint32_t) * 2 * d);
    if (by_residual) {
      w_lists.ensure(sizeof(int64_t) * rows);
      w_D.ensure(sizeof(float) * rows);
    }
    uint32_t* lo = w_mm.as<uint32_t>();
    uint32_t* hi = lo + d;
    launch_sq_minmax_init(lo, hi, d, stream);
    std::vector<float> stage;
    for (int64_t r0 = 0; r0 < m; r0 += rows) {
      const int64_t c = std::min(rows, m - r0);
      const float* src = x + r0 * d;
      if (!pick.empty()) {
        stage.resize((size_t)c * d);
        for (int64_t i = 0; i < c; i++) std::memcpy(&stage[(size_t)i * d], x + pick[r0 + i] * d, sizeof(float) * d);
        src = stage.data();
      }
      float* xd = w_xa.as<float>();
      HIPCHECK(hipMemcpyAsync(xd, src, sizeof(float) * c * d, hipMemcpyHostToDevice, stream));
      if (by_residual) {
        cq.launch(cw, xd, c, 1, w_D.as<float>(), w_lists.as<int64_t>(), stream);
        launch_ivfsq_residuals(xd, c, 1, d, w_lists.as<int64_t>(), cq.d_cent.as<float>(), nlist, xd, stream);
      }
      launch_sq_minmax(xd, c, d, lo, hi, stream);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipStreamSynchronize(stream));  // w_xa and stage are reused
    }
    std::vector<uint32_t> bits(2 * (size_t)d);
    HIPCHECK(hipMemcpyAsync(bits.data(), w_mm.p, sizeof(uint32_t) * 2 * d, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
    params = sq_trained_from_minmax(bits, qtype, d);
    upload_params();
  }

  // n vectors (host or device) into the pending set: assigned by the search's coarse kernels
  // (top-1) and encoded there, pass by pass.  Merged into the image before the lists are
  // next read, or once the pending set is as large as the image (and at least kChunkBytes).
  void add_dev(int64_t n, const float* x, bool x_on_device, const int64_t* ids, bool ids_on_device, hipStream_t s) {
    if (n <= 0) return;
    reserve_pending(n, s);
    const int64_t rows = chunk_rows(n, true);
    if (!x_on_device) w_xa.ensure(sizeof(float) * rows * d);
    w_D.ensure(sizeof(float) * rows);
    int64_t* lists = q.lists.as<int64_t>() + q.n;
    uint8_t* codes = q.rows.as<uint8_t>() + q.n * code_size;
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      const float* xd = x + r0 * d;
      if (!x_on_device) {
        HIPCHECK(hipMemcpyAsync(w_xa.p, xd, sizeof(float) * c * d, hipMemcpyHostToDevice, s));
        xd = w_xa.as<float>();
      }
      cq.launch(cw, xd, c, 1, w_D.as<float>(), lists + r0, s);
      launch_ivfsq_encode(codec, xd, c, d, lists + r0, cq.d_cent.as<float>(), nlist, by_residual,
                          d_vmin.as<float>(), d_vdiff.as<float>(), codes + r0 * code_size, s);
      HIPCHECK(hipGetLastError());
      if (!x_on_device) HIPCHECK(hipStreamSynchronize(s));  // w_xa is reused
    }
    pending_ids(n, ids, ids_on_device, s);
    commit_pending(n, s);
  }

  // n precomputed codes with their lists and labels (host) into the pending set
  void add_codes(int64_t n, const int64_t* lists, const uint8_t* codes, const int64_t* ids) {
    if (n <= 0) return;
    reserve_pending(n, stream);
    HIPCHECK(hipMemcpyAsync(q.lists.as<int64_t>() + q.n, lists, sizeof(int64_t) * n, hipMemcpyHostToDevice, stream));
    HIPCHECK(hipMemcpyAsync(q.rows.as<uint8_t>() + q.n * code_size, codes, row_bytes() * n, hipMemcpyHostToDevice,
                            stream));
    pending_ids(n, ids, false, stream);
    commit_pending(n, stream);
  }
};

extern "C" {

int ivfpq_ivfsq_create(int d, int nlist, int qtype, int metric, int by_residual, int device,
                       ivfpq_ivfsq_index** out) {
  return guarded([&] {
    check_ivf_create("IndexIVFScalarQuantizer", out, d, nlist);
    check_sq_qtype(qtype);
    check_ivf_device(metric, device);
    DeviceGuard g(device);
    auto h = std::make_unique<ivfpq_ivfsq_index>();
    h->qtype = qtype;
    h->codec = sq_codec_of(qtype);
    h->code_size = sq_code_size(h->codec, d);
    h->by_residual = by_residual != 0;
    h->sq_trained = qtype == IVFPQ_SQ_FP16;  // no table to train
    // (the scan's 16-byte loads may straddle the last row's end: kSqScanSlack)
    h->open("IndexIVFScalarQuantizer", d, nlist, metric, device, (size_t)h->code_size, kSqScanSlack);
    *out = h.release();
  });
}

int ivfpq_ivfsq_free(ivfpq_ivfsq_index* h) { return free_handle(h); }

int ivfpq_ivfsq_train(ivfpq_ivfsq_index* h, int64_t n, const float* x, int niter, uint64_t seed) {
  return with_handle(h, [&] {
    require(x != nullptr && n > 0, "empty training set");
    h->quiesce();
    std::vector<float> cent((size_t)h->nlist * h->d);
    KMeans(h->stream).kmeans(x, n, h->d, h->nlist, niter, seed, cent.data(), h->ip());  // ivfpq_ivfflat_train's
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->centroids = std::move(cent);
    h->upload_centroids();
    h->train_sq(n, x);
  });
}

int ivfpq_ivfsq_set_trained(ivfpq_ivfsq_index* h, const float* centroids, const float* sq_trained, int64_t count) {
  return with_handle(h, [&] {
    require(centroids != nullptr, "null centroids");
    const int64_t want = (int64_t)sq_nparams(h->qtype, h->d);
    require(count == want, "trained has " + std::to_string(count) + " values, this quantizer " + std::to_string(want));
    require(count == 0 || sq_trained != nullptr, "null trained");
    h->centroids.assign(centroids, centroids + (size_t)h->nlist * h->d);
    h->upload_centroids();
    h->params.assign(sq_trained, sq_trained + count);
    h->upload_params();
  });
}

int ivfpq_ivfsq_add(ivfpq_ivfsq_index* h, int64_t n, const float* x, const int64_t* ids) {
  return with_handle(h, [&] {
    require(h->trained(), "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, false, ids, false, h->stream);
  });
}

int ivfpq_ivfsq_add_device(ivfpq_ivfsq_index* h, int64_t n, const float* x, const int64_t* ids, void* stream) {
  return with_handle(h, [&] {
    require(h->trained(), "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, true, ids, true, stream ? (hipStream_t)stream : h->stream);
  });
}

int ivfpq_ivfsq_add_codes(ivfpq_ivfsq_index* h, int64_t n, const int64_t* lists, const uint8_t* codes,
                          const int64_t* ids) {
  return with_handle(h, [&] {
    require(h->trained(), "index is not trained");
    if (n <= 0) return;
    require(lists != nullptr && codes != nullptr, "null lists / codes");
    for (int64_t i = 0; i < n; i++) require(lists[i] >= 0 && lists[i] < h->nlist, "list id out of range");
    h->add_codes(n, lists, codes, ids);
  });
}

int ivfpq_ivfsq_reset(ivfpq_ivfsq_index* h) { return ivf_reset(h); }

int ivfpq_ivfsq_set_nprobe(ivfpq_ivfsq_index* h, int nprobe) { return ivf_set_nprobe(h, nprobe); }

int ivfpq_ivfsq_get_nprobe(const ivfpq_ivfsq_index* h) { return ivf_get_nprobe(h); }

int ivfpq_ivfsq_search(ivfpq_ivfsq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I) {
  return ivf_search(h, n, x, k, D, I);
}

int ivfpq_ivfsq_search_preassigned(ivfpq_ivfsq_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                   const float* Dq, float* D, int64_t* I) {
  return ivf_search_preassigned(h, n, x, k, Iq, Dq, D, I);
}

int ivfpq_ivfsq_search_device(ivfpq_ivfsq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I,
                              void* stream) {
  return ivf_search_device(h, n, x, k, D, I, stream);
}

int ivfpq_ivfsq_search_preassigned_device(ivfpq_ivfsq_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                          const float* Dq, float* D, int64_t* I, void* stream) {
  return ivf_search_preassigned_device(h, n, x, k, Iq, Dq, D, I, stream);
}

int64_t ivfpq_ivfsq_ntotal(const ivfpq_ivfsq_index* h) { return ivf_ntotal(h); }

int ivfpq_ivfsq_is_trained(const ivfpq_ivfsq_index* h) { return h && h->trained() ? 1 : 0; }

int ivfpq_ivfsq_get_dims(const ivfpq_ivfsq_index* h, int* d, int* nlist, int* qtype, int* metric, int* by_residual,
                         int* code_size) {
  return guarded([&] {
    check_handle(h);
    if (d) *d = h->d;
    if (nlist) *nlist = h->nlist;
    if (qtype) *qtype = h->qtype;
    if (metric) *metric = h->metric;
    if (by_residual) *by_residual = h->by_residual ? 1 : 0;
    if (code_size) *code_size = h->code_size;
  });
}

int ivfpq_ivfsq_get_centroids(const ivfpq_ivfsq_index* h, float* out) { return ivf_get_centroids(h, out); }

int ivfpq_ivfsq_get_trained(const ivfpq_ivfsq_index* h, float* out, int64_t* count) {
  return guarded([&] {
    check_handle(h);
    require(h->trained(), "index is not trained");
    if (count) *count = (int64_t)h->params.size();
    if (out && !h->params.empty()) std::memcpy(out, h->params.data(), sizeof(float) * h->params.size());
  });
}

int ivfpq_ivfsq_get_list_sizes(ivfpq_ivfsq_index* h, int64_t* out) { return ivf_get_list_sizes(h, out); }

int ivfpq_ivfsq_get_list(ivfpq_ivfsq_index* h, int list, uint8_t* codes, int64_t* ids) {
  return ivf_get_list(h, list, codes, ids);
}

}  // extern "C"
