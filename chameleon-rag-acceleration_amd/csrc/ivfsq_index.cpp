// IVF over scalar-quantizer codes (IndexIVFScalarQuantizer) behind the C-ABI of include/ivfpq.h.
// faiss.IndexIVFScalarQuantizer: IVF-Flat's coarse quantizer, device list image and pending-add
// merge (ivfflat_index.cpp) with the rows stored as the flat scalar quantizer's fp16 / 8-bit
// codes (sq_index.cpp), of the vector or, by_residual, of the vector minus its list's
// centroid; scanned by ivf_sq.hip.  The codes live only in the device image {list_off, codes,
// ids}, every list sorted by label, with the scan's read slack behind the last row; adds are
// encoded straight into a pending set on the device and merged with the image kernels of
// ivfpq_build.h at code size d or 2 d.  Device calls on different streams are ordered one
// after the other (one workspace per handle).
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "coarse_quantizer.h"
#include "ivf_sq.h"
#include "ivfpq.h"
#include "kmeans.h"
#include "list_image.h"
#include "sq_params.h"

using namespace chivf;

namespace {
constexpr int64_t kSqTrainRows = 100000;  // ScalarQuantizer::train_residual's subsample
constexpr uint64_t kSqTrainSeed = 1234;   // ... and its rand_perm seed
}  // namespace

struct ivfpq_ivfsq_index : StreamOrder {
  int d = 0, nlist = 0, qtype = IVFPQ_SQ_FP16, metric = IVFPQ_METRIC_L2, device = 0;
  int codec = SQ_CODEC_FP16, code_size = 0;
  bool by_residual = true;
  int nprobe = 1;
  bool cent_trained = false, sq_trained = false;
  std::vector<float> centroids;  // [nlist][d]
  std::vector<float> params;     // Faiss's sq.trained
  CoarseQuantizer cq;
  CoarseScratch cw;
  DevBuf d_vmin, d_vdiff;
  int64_t ntotal = 0, next_id = 0;
  int64_t img_n = 0;  // codes in the image (ntotal = img_n + q.n)
  ListImage img;
  std::vector<int64_t> h_off;      // the image's list offsets
  std::vector<int64_t> range_top;  // range_top[p] = row ranges of the p longest lists (the slot bound)
  PendingSet q;                    // pending adds: list numbers, labels, codes
  DevBuf w_D, w_x, w_xa, w_mm, h_D, h_I, h_Iq, h_Dq;  // add / train scratch; staging of the host entry points
  DevBuf w_lists, w_dis, w_cd, p_cnt, p_bucket, p_probe, p_qr, p_items, p_used, p_tau, p_partD, p_partI, p_tmpD,
      p_tmpI;
  hipStream_t stream = nullptr;
  std::mutex mu;

  ~ivfpq_ivfsq_index() {
    if (stream) (void)hipStreamDestroy(stream);
  }
  bool ip() const { return metric == IVFPQ_METRIC_INNER_PRODUCT; }
  bool trained() const { return cent_trained && sq_trained; }
  size_t row_bytes() const { return q.row_bytes; }

  void upload_centroids() {
    quiesce();
    cq.upload(centroids.data(), stream);
    cent_trained = true;
  }
  void upload_params() {
    quiesce();
    if (codec == SQ_CODEC_8BIT) sq_upload_params(params, qtype, d, d_vmin, d_vdiff, stream);
    sq_trained = true;
  }

  void set_offsets(std::vector<int64_t> off) {
    h_off = std::move(off);
    std::vector<int64_t> r(nlist);
    for (int l = 0; l < nlist; l++) r[l] = (h_off[l + 1] - h_off[l] + kIvfFlatRangeRows - 1) / kIvfFlatRangeRows;
    std::sort(r.begin(), r.end(), std::greater<int64_t>());
    range_top.assign(nlist + 1, 0);
    for (int l = 0; l < nlist; l++) range_top[l + 1] = range_top[l] + r[l];
  }

  // an empty image (create, reset)
  void clear_image() {
    quiesce();
    q.drop();
    img.rows.release();
    img.ids.release();
    img.off.ensure(sizeof(int64_t) * (nlist + 1));
    HIPCHECK(hipMemsetAsync(img.off.p, 0, sizeof(int64_t) * (nlist + 1), stream));
    HIPCHECK(hipStreamSynchronize(stream));
    set_offsets(std::vector<int64_t>(nlist + 1, 0));
    img_n = ntotal = next_id = 0;
  }

  // rows per pass of add and train: the [rows][nlist] coarse keys and the [rows][d] staging within kChunkBytes
  int64_t chunk_rows(int64_t n) const {
    const int64_t by_keys =
        nlist >= kSegmentedNlist ? (int64_t)1 << 18 : (int64_t)(kChunkBytes / ((size_t)nlist * 4));
    return std::max<int64_t>(1, std::min<int64_t>({n, by_keys, (int64_t)(kChunkBytes / (sizeof(float) * d))}));
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
    const int64_t rows = chunk_rows(m);
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

  void reserve_pending(int64_t n, hipStream_t s) {
    require(ntotal + n < (int64_t)INT32_MAX, "IndexIVFScalarQuantizer holds fewer than 2^31 - 1 vectors");
    order_after(s);
    quiesce();
    q.reserve(q.n + n, s);
  }
  void commit_pending(int64_t n, hipStream_t s) {
    HIPCHECK(hipStreamSynchronize(s));
    q.n += n;
    ntotal += n;
    if (q.n >= std::max<int64_t>(img_n, (int64_t)(kChunkBytes / row_bytes()))) flush_pending(s);
  }
  void pending_ids(int64_t n, const int64_t* ids, bool ids_on_device, hipStream_t s) {
    if (!ids) {
      launch_iota_i64(q.ids.as<int64_t>() + q.n, n, next_id, s);
      next_id += n;
    } else {
      HIPCHECK(hipMemcpyAsync(q.ids.as<int64_t>() + q.n, ids, sizeof(int64_t) * n,
                              ids_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    }
  }

  // n vectors (host or device) into the pending set: assigned by the search's coarse kernels
  // (top-1) and encoded there, pass by pass.  Merged into the image before the lists are
  // next read, or once the pending set is as large as the image (and at least kChunkBytes).
  void add_dev(int64_t n, const float* x, bool x_on_device, const int64_t* ids, bool ids_on_device, hipStream_t s) {
    if (n <= 0) return;
    reserve_pending(n, s);
    const int64_t rows = chunk_rows(n);
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

  // the pending codes merged into the image (merge_pending with code_size bytes as the row;
  // the new image is allocated with the scan's slack behind its last row)
  void flush_pending(hipStream_t s) {
    if (q.n == 0) return;
    quiesce();
    set_offsets(merge_pending(q, img, nlist, 0, nlist, h_off.data(), q.n,
                              "pending merge: a vector was assigned to no list", s));
    img_n = h_off[nlist];
    require(img_n == ntotal, "pending merge: image size disagrees with ntotal");
  }

  // The search on device pointers, on stream s.  Iq non-null = preassigned probes [n][nprobe]
  // (the handle's nprobe) with their coarse values Dq (read for the inner product with
  // by_residual only; null = zeros).
  void search_dev(int64_t n, const float* x, int k, float* D, int64_t* I, const int64_t* Iq, const float* Dq,
                  hipStream_t s) {
    flush_pending(s);
    if (n == 0) return;
    order_after(s);
    if (img_n == 0) {
      launch_fill_empty(D, I, n * k, ip(), s);
      HIPCHECK(hipGetLastError());
      mark_done(s);
      return;
    }
    const int np = Iq ? nprobe : std::min(nprobe, nlist);
    const IvfFlatPlan pl = ivfsq_plan(codec, k, range_top[std::min(np, nlist)]);
    const bool resid_q = by_residual && !ip();  // residual queries
    const bool coarse_add = by_residual && ip();  // the pair's coarse value added
    // queries per chunk: the [c][nlist] coarse keys, buckets and probe columns and the
    // [c][np][d] residual queries within kChunkBytes each, the partial lists (12 bytes per
    // entry, and the first merge round's output) within kPartialBytes
    const size_t part_q = (size_t)pl.S * k * 12 * 2;
    int64_t qc = std::max<int64_t>(
        1, std::min<int64_t>({n, (int64_t)(kChunkBytes / ((size_t)nlist * (by_residual ? 12 : 8))),
                              (int64_t)(kPartialBytes / part_q), (int64_t)(INT32_MAX / 2) / ((int64_t)pl.S * k)}));
    if (resid_q) qc = std::max<int64_t>(1, std::min<int64_t>(qc, (int64_t)(kChunkBytes / (sizeof(float) * np * d))));
    if (!Iq) {
      w_lists.ensure(sizeof(int64_t) * qc * np);
      w_dis.ensure(sizeof(float) * qc * np);
    } else if (coarse_add && !Dq) {
      w_cd.ensure(sizeof(float) * qc * np);
      HIPCHECK(hipMemsetAsync(w_cd.p, 0, sizeof(float) * qc * np, s));
    }
    p_cnt.ensure(sizeof(int32_t) * nlist);
    p_bucket.ensure(sizeof(int2) * (size_t)nlist * qc);
    if (by_residual) p_probe.ensure(sizeof(int32_t) * (size_t)nlist * qc);
    if (resid_q) p_qr.ensure(sizeof(float) * (size_t)qc * np * d);
    p_items.ensure(sizeof(int32_t) * (nlist + 1));
    p_used.ensure(sizeof(int32_t) * qc);
    p_tau.ensure(sizeof(uint32_t) * qc);
    p_partD.ensure(sizeof(float) * (size_t)pl.S * qc * k);
    p_partI.ensure(sizeof(int64_t) * (size_t)pl.S * qc * k);
    const size_t tmp_lists = (size_t)std::max(1, pl.S / pl.fan);
    p_tmpD.ensure(sizeof(float) * tmp_lists * qc * k);
    p_tmpI.ensure(sizeof(int64_t) * tmp_lists * qc * k);
    for (int64_t q0 = 0; q0 < n; q0 += qc) {
      const int64_t c = std::min(qc, n - q0);
      const float* xq = x + q0 * d;
      IvfSqArgs a;
      IvfFlatArgs& f = a.f;
      f.x = xq;
      f.nq = c;
      f.d = d;
      f.vecs = nullptr;
      f.ids = img.ids.as<int64_t>();
      f.list_off = img.off.as<int64_t>();
      f.nlist = nlist;
      a.cdis = nullptr;
      if (Iq) {
        f.probes = Iq + q0 * np;
        if (coarse_add) a.cdis = Dq ? Dq + q0 * np : w_cd.as<float>();
      } else {
        cq.launch(cw, xq, c, np, w_dis.as<float>(), w_lists.as<int64_t>(), s);
        f.probes = w_lists.as<int64_t>();
        if (coarse_add) a.cdis = w_dis.as<float>();
      }
      f.nprobe = np;
      f.dedup = Iq != nullptr;
      f.k = k;
      f.ip = ip();
      f.cnt = p_cnt.as<int32_t>();
      f.bucket = p_bucket.as<int2>();
      f.item_off = p_items.as<int32_t>();
      f.used = p_used.as<int32_t>();
      f.tau = p_tau.as<uint32_t>();
      f.partD = p_partD.as<float>();
      f.partI = p_partI.as<int64_t>();
      f.tmpD = p_tmpD.as<float>();
      f.tmpI = p_tmpI.as<int64_t>();
      f.D = D + q0 * k;
      f.I = I + q0 * k;
      a.codec = codec;
      a.codes = img.rows.as<uint8_t>();
      a.vmin = d_vmin.as<float>();
      a.vdiff = d_vdiff.as<float>();
      a.by_residual = by_residual;
      a.cent = cq.d_cent.as<float>();
      a.probe_of = p_probe.as<int32_t>();
      a.qr = p_qr.as<float>();
      launch_ivfsq_search(a, pl, s);
      HIPCHECK(hipGetLastError());
    }
    mark_done(s);
  }

  // host-buffer search (copies in and out on the handle's stream)
  void search_host(int64_t n, const float* x, int k, float* D, int64_t* I, const int64_t* Iq, const float* Dq) {
    if (n == 0) return;
    quiesce();
    w_x.ensure(sizeof(float) * n * d);
    h_D.ensure(sizeof(float) * n * k);
    h_I.ensure(sizeof(int64_t) * n * k);
    HIPCHECK(hipMemcpyAsync(w_x.p, x, sizeof(float) * n * d, hipMemcpyHostToDevice, stream));
    if (Iq) {
      h_Iq.ensure(sizeof(int64_t) * n * nprobe);
      HIPCHECK(hipMemcpyAsync(h_Iq.p, Iq, sizeof(int64_t) * n * nprobe, hipMemcpyHostToDevice, stream));
    }
    if (Iq && Dq) {
      h_Dq.ensure(sizeof(float) * n * nprobe);
      HIPCHECK(hipMemcpyAsync(h_Dq.p, Dq, sizeof(float) * n * nprobe, hipMemcpyHostToDevice, stream));
    }
    search_dev(n, w_x.as<float>(), k, h_D.as<float>(), h_I.as<int64_t>(), Iq ? h_Iq.as<int64_t>() : nullptr,
               Iq && Dq ? h_Dq.as<float>() : nullptr, stream);
    HIPCHECK(hipMemcpyAsync(D, h_D.p, sizeof(float) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipMemcpyAsync(I, h_I.p, sizeof(int64_t) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
};

namespace {
// the search arguments, in the words of ivfpq_search
void check_ivfsq_search(const ivfpq_ivfsq_index* h, int64_t n, const void* x, int k, const void* D, const void* I) {
  check_search_args(h->trained(), n, k);
  require(n == 0 || (x && D && I), "null buffer");
}
}  // namespace

extern "C" {

int ivfpq_ivfsq_create(int d, int nlist, int qtype, int metric, int by_residual, int device,
                       ivfpq_ivfsq_index** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    require(d >= 4 && d <= 2048 && d % 4 == 0,
            "IndexIVFScalarQuantizer: d must be a multiple of 4 in [4, 2048] (d = " + std::to_string(d) + ")");
    require(nlist >= 1, "nlist must be >= 1");
    check_sq_qtype(qtype);
    require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT, "unknown metric");
    int ndev = 0;
    HIPCHECK(hipGetDeviceCount(&ndev));
    require(device >= 0 && device < ndev, "device ordinal out of range");
    DeviceGuard g(device);
    auto h = std::make_unique<ivfpq_ivfsq_index>();
    h->d = h->cq.d = d;
    h->nlist = h->cq.nlist = nlist;
    h->metric = h->cq.metric = metric;
    h->qtype = qtype;
    h->codec = sq_codec_of(qtype);
    h->code_size = sq_code_size(h->codec, d);
    h->by_residual = by_residual != 0;
    h->device = device;
    h->q.row_bytes = (size_t)h->code_size;
    h->q.image_slack = kSqScanSlack;  // the scan's 16-byte loads may straddle the last row's end
    h->sq_trained = qtype == IVFPQ_SQ_FP16;  // no table to train
    HIPCHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->create();
    h->clear_image();
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

int ivfpq_ivfsq_reset(ivfpq_ivfsq_index* h) {
  return with_handle(h, [&] { h->clear_image(); });
}

int ivfpq_ivfsq_set_nprobe(ivfpq_ivfsq_index* h, int nprobe) {
  return guarded([&] {
    check_handle(h);
    require(nprobe >= 1 && nprobe <= kMaxK, "nprobe must be in [1, " + std::to_string(kMaxK) + "]");
    h->nprobe = nprobe;
  });
}

int ivfpq_ivfsq_get_nprobe(const ivfpq_ivfsq_index* h) { return h ? h->nprobe : -1; }

int ivfpq_ivfsq_search(ivfpq_ivfsq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I) {
  return with_handle(h, [&] {
    check_ivfsq_search(h, n, x, k, D, I);
    h->search_host(n, x, k, D, I, nullptr, nullptr);
  });
}

int ivfpq_ivfsq_search_preassigned(ivfpq_ivfsq_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                   const float* Dq, float* D, int64_t* I) {
  return with_handle(h, [&] {
    check_ivfsq_search(h, n, x, k, D, I);
    require(n == 0 || Iq, "null Iq");
    for (int64_t i = 0; i < n * h->nprobe; i++) require(Iq[i] < h->nlist, "list id out of range in Iq");
    h->search_host(n, x, k, D, I, Iq, Dq);
  });
}

int ivfpq_ivfsq_search_device(ivfpq_ivfsq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I,
                              void* stream) {
  return with_handle(h, [&] {
    check_ivfsq_search(h, n, x, k, D, I);
    h->search_dev(n, x, k, D, I, nullptr, nullptr, (hipStream_t)stream);
  });
}

int ivfpq_ivfsq_search_preassigned_device(ivfpq_ivfsq_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                          const float* Dq, float* D, int64_t* I, void* stream) {
  return with_handle(h, [&] {
    check_ivfsq_search(h, n, x, k, D, I);
    require(n == 0 || Iq, "null Iq");
    h->search_dev(n, x, k, D, I, n ? Iq : nullptr, Dq, (hipStream_t)stream);
  });
}

int64_t ivfpq_ivfsq_ntotal(const ivfpq_ivfsq_index* h) { return h ? h->ntotal : -1; }

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

int ivfpq_ivfsq_get_centroids(const ivfpq_ivfsq_index* h, float* out) {
  return guarded([&] {
    check_handle(h);
    require(h->cent_trained, "index is not trained");
    require(out != nullptr, "null output pointer");
    std::memcpy(out, h->centroids.data(), sizeof(float) * h->centroids.size());
  });
}

int ivfpq_ivfsq_get_trained(const ivfpq_ivfsq_index* h, float* out, int64_t* count) {
  return guarded([&] {
    check_handle(h);
    require(h->trained(), "index is not trained");
    if (count) *count = (int64_t)h->params.size();
    if (out && !h->params.empty()) std::memcpy(out, h->params.data(), sizeof(float) * h->params.size());
  });
}

int ivfpq_ivfsq_get_list_sizes(ivfpq_ivfsq_index* h, int64_t* out) {
  return with_handle(h, [&] {
    require(out != nullptr, "null output pointer");
    h->flush_pending(h->stream);
    for (int l = 0; l < h->nlist; l++) out[l] = h->h_off[l + 1] - h->h_off[l];
  });
}

int ivfpq_ivfsq_get_list(ivfpq_ivfsq_index* h, int list, uint8_t* codes, int64_t* ids) {
  return with_handle(h, [&] {
    require(list >= 0 && list < h->nlist, "list id out of range");
    h->flush_pending(h->stream);
    h->quiesce();
    const int64_t b = h->h_off[list], n = h->h_off[list + 1] - b;
    if (n == 0) return;
    if (codes)
      HIPCHECK(hipMemcpyAsync(codes, h->img.rows.as<uint8_t>() + b * h->code_size, h->row_bytes() * n,
                              hipMemcpyDeviceToHost, h->stream));
    if (ids)
      HIPCHECK(hipMemcpyAsync(ids, h->img.ids.as<int64_t>() + b, sizeof(int64_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  });
}

}  // extern "C"
