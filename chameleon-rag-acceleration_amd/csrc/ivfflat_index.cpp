// IVF-Flat (IndexIVFFlat) behind the C-ABI of include/ivfpq.h.
// faiss.IndexIVFFlat: IVF-PQ's coarse quantizer (k-means, matrix-core keys,
// top-nprobe selection) over inverted lists of the raw fp32 vectors, scanned by
// ivf_flat.hip.  The vectors live only in the device image {list_off, vectors, ids},
// every list sorted by label; adds wait in a pending set on the device and are merged
// with the image kernels of ivfpq_build.h at code size 4 d.  Device calls on different
// streams are ordered one after the other (one workspace per handle).
#include <cstring>
#include <functional>
#include <memory>
#include <vector>

#include "coarse_quantizer.h"
#include "ivf_flat.h"
#include "ivfpq.h"
#include "kmeans.h"
#include "list_image.h"

using namespace chivf;

struct ivfpq_ivfflat_index : StreamOrder {
  int d = 0, nlist = 0, metric = IVFPQ_METRIC_L2, device = 0;
  int nprobe = 1;
  bool trained = false;
  std::vector<float> centroids;  // [nlist][d]
  CoarseQuantizer cq;
  CoarseScratch cw;
  int64_t ntotal = 0, next_id = 0;
  int64_t img_n = 0;  // vectors in the image (ntotal = img_n + q.n)
  ListImage img;
  std::vector<int64_t> h_off;      // the image's list offsets
  std::vector<int64_t> range_top;  // range_top[p] = row ranges of the p longest lists (the slot bound)
  PendingSet q;                    // pending adds: list numbers, labels, vectors
  DevBuf w_D, w_x, h_D, h_I, h_Iq;  // add scratch; staging of the host entry points
  DevBuf w_lists, w_dis, p_cnt, p_bucket, p_items, p_used, p_tau, p_partD, p_partI, p_tmpD, p_tmpI;
  hipStream_t stream = nullptr;
  std::mutex mu;

  ~ivfpq_ivfflat_index() {
    if (stream) (void)hipStreamDestroy(stream);
  }
  bool ip() const { return metric == IVFPQ_METRIC_INNER_PRODUCT; }
  size_t row_bytes() const { return q.row_bytes; }

  void upload_centroids() {
    quiesce();
    cq.upload(centroids.data(), stream);
    trained = true;
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

  // n vectors (host or device) into the pending set: copied behind it, then assigned
  // there by the search's coarse kernels (top-1), as IVF-PQ's add_dev assigns.
  // Merged into the image before the lists are next read, or once the pending set is
  // as large as the image (and at least kChunkBytes), so that a sequence of adds
  // moves every vector O(1) times.
  void add_dev(int64_t n, const float* x, bool x_on_device, const int64_t* ids, bool ids_on_device, hipStream_t s) {
    require(trained, "index is not trained");
    if (n <= 0) return;
    require(ntotal + n < (int64_t)INT32_MAX, "IndexIVFFlat holds fewer than 2^31 - 1 vectors");
    order_after(s);
    quiesce();
    const int64_t rows = nlist >= kSegmentedNlist ? std::min<int64_t>(n, 1 << 18)
                                                  : std::max<int64_t>(1, std::min<int64_t>(n, kChunkBytes / ((size_t)nlist * 4)));
    q.reserve(q.n + n, s);
    float* xd = q.rows.as<float>() + q.n * d;
    int64_t* lists = q.lists.as<int64_t>() + q.n;
    HIPCHECK(hipMemcpyAsync(xd, x, row_bytes() * n, x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    w_D.ensure(sizeof(float) * rows);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      cq.launch(cw, xd + r0 * d, c, 1, w_D.as<float>(), lists + r0, s);
      HIPCHECK(hipGetLastError());
    }
    if (!ids) {
      launch_iota_i64(q.ids.as<int64_t>() + q.n, n, next_id, s);
      next_id += n;
    } else {
      HIPCHECK(hipMemcpyAsync(q.ids.as<int64_t>() + q.n, ids, sizeof(int64_t) * n,
                              ids_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    q.n += n;
    ntotal += n;
    if (q.n >= std::max<int64_t>(img_n, (int64_t)(kChunkBytes / row_bytes()))) flush_pending(s);
  }

  // the pending vectors merged into the image (merge_pending with the vector's 4 d bytes as the row)
  void flush_pending(hipStream_t s) {
    if (q.n == 0) return;
    quiesce();
    set_offsets(merge_pending(q, img, nlist, 0, nlist, h_off.data(), q.n,
                              "pending merge: a vector was assigned to no list", s));
    img_n = h_off[nlist];
    require(img_n == ntotal, "pending merge: image size disagrees with ntotal");
  }

  // The search on device pointers, on stream s.  Iq non-null = preassigned probes
  // [n][nprobe] (the handle's nprobe, as ivfpq_search_preassigned).
  void search_dev(int64_t n, const float* x, int k, float* D, int64_t* I, const int64_t* Iq, hipStream_t s) {
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
    const IvfFlatPlan pl = ivfflat_plan(k, range_top[std::min(np, nlist)]);
    // queries per chunk: the [c][nlist] coarse keys and buckets within kChunkBytes, the
    // partial lists (12 bytes per entry, and the first merge round's output) within kPartialBytes
    const size_t part_q = (size_t)pl.S * k * 12 * 2;
    const int64_t qc = std::max<int64_t>(
        1, std::min<int64_t>({n, (int64_t)(kChunkBytes / ((size_t)nlist * 8)), (int64_t)(kPartialBytes / part_q),
                              (int64_t)(INT32_MAX / 2) / ((int64_t)pl.S * k)}));
    if (!Iq) {
      w_lists.ensure(sizeof(int64_t) * qc * np);
      w_dis.ensure(sizeof(float) * qc * np);
    }
    p_cnt.ensure(sizeof(int32_t) * nlist);
    p_bucket.ensure(sizeof(int2) * (size_t)nlist * qc);
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
      IvfFlatArgs a;
      a.x = xq;
      a.nq = c;
      a.d = d;
      a.vecs = img.rows.as<float>();
      a.ids = img.ids.as<int64_t>();
      a.list_off = img.off.as<int64_t>();
      a.nlist = nlist;
      if (Iq) {
        a.probes = Iq + q0 * np;
      } else {
        cq.launch(cw, xq, c, np, w_dis.as<float>(), w_lists.as<int64_t>(), s);
        a.probes = w_lists.as<int64_t>();
      }
      a.nprobe = np;
      a.dedup = Iq != nullptr;
      a.k = k;
      a.ip = ip();
      a.cnt = p_cnt.as<int32_t>();
      a.bucket = p_bucket.as<int2>();
      a.item_off = p_items.as<int32_t>();
      a.used = p_used.as<int32_t>();
      a.tau = p_tau.as<uint32_t>();
      a.partD = p_partD.as<float>();
      a.partI = p_partI.as<int64_t>();
      a.tmpD = p_tmpD.as<float>();
      a.tmpI = p_tmpI.as<int64_t>();
      a.D = D + q0 * k;
      a.I = I + q0 * k;
      launch_ivfflat_search(a, pl, s);
      HIPCHECK(hipGetLastError());
    }
    mark_done(s);
  }

  // host-buffer search (copies in and out on the handle's stream)
  void search_host(int64_t n, const float* x, int k, float* D, int64_t* I, const int64_t* Iq) {
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
    search_dev(n, w_x.as<float>(), k, h_D.as<float>(), h_I.as<int64_t>(), Iq ? h_Iq.as<int64_t>() : nullptr, stream);
    HIPCHECK(hipMemcpyAsync(D, h_D.p, sizeof(float) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipMemcpyAsync(I, h_I.p, sizeof(int64_t) * n * k, hipMemcpyDeviceToHost, stream));
    HIPCHECK(hipStreamSynchronize(stream));
  }
};

namespace {
// the search arguments, in the words of ivfpq_search
void check_ivfflat_search(const ivfpq_ivfflat_index* h, int64_t n, const void* x, int k, const void* D,
                          const void* I) {
  check_search_args(h->trained, n, k);
  require(n == 0 || (x && D && I), "null buffer");
}
}  // namespace

extern "C" {

int ivfpq_ivfflat_create(int d, int nlist, int metric, int device, ivfpq_ivfflat_index** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    require(d >= 4 && d <= 2048 && d % 4 == 0,
            "IndexIVFFlat: d must be a multiple of 4 in [4, 2048] (d = " + std::to_string(d) + ")");
    require(nlist >= 1, "nlist must be >= 1");
    require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT, "unknown metric");
    int ndev = 0;
    HIPCHECK(hipGetDeviceCount(&ndev));
    require(device >= 0 && device < ndev, "device ordinal out of range");
    DeviceGuard g(device);
    auto h = std::make_unique<ivfpq_ivfflat_index>();
    h->d = h->cq.d = d;
    h->nlist = h->cq.nlist = nlist;
    h->metric = h->cq.metric = metric;
    h->device = device;
    h->q.row_bytes = sizeof(float) * (size_t)d;
    HIPCHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    h->create();
    h->clear_image();
    *out = h.release();
  });
}

int ivfpq_ivfflat_free(ivfpq_ivfflat_index* h) { return free_handle(h); }

int ivfpq_ivfflat_train(ivfpq_ivfflat_index* h, int64_t n, const float* x, int niter, uint64_t seed) {
  return with_handle(h, [&] {
    require(x != nullptr && n > 0, "empty training set");
    h->quiesce();
    std::vector<float> cent((size_t)h->nlist * h->d);
    KMeans(h->stream).kmeans(x, n, h->d, h->nlist, niter, seed, cent.data(), h->ip());  // ivfpq_train's coarse stage
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->centroids = std::move(cent);
    h->upload_centroids();
  });
}

int ivfpq_ivfflat_set_trained(ivfpq_ivfflat_index* h, const float* centroids) {
  return with_handle(h, [&] {
    require(centroids != nullptr, "null centroids");
    h->centroids.assign(centroids, centroids + (size_t)h->nlist * h->d);
    h->upload_centroids();
  });
}

int ivfpq_ivfflat_add(ivfpq_ivfflat_index* h, int64_t n, const float* x, const int64_t* ids) {
  return with_handle(h, [&] {
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, false, ids, false, h->stream);
  });
}

int ivfpq_ivfflat_add_device(ivfpq_ivfflat_index* h, int64_t n, const float* x, const int64_t* ids, void* stream) {
  return with_handle(h, [&] {
    require(h->trained, "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, true, ids, true, stream ? (hipStream_t)stream : h->stream);
  });
}

int ivfpq_ivfflat_reset(ivfpq_ivfflat_index* h) {
  return with_handle(h, [&] { h->clear_image(); });
}

int ivfpq_ivfflat_set_nprobe(ivfpq_ivfflat_index* h, int nprobe) {
  return guarded([&] {
    check_handle(h);
    require(nprobe >= 1 && nprobe <= kMaxK, "nprobe must be in [1, " + std::to_string(kMaxK) + "]");
    h->nprobe = nprobe;
  });
}

int ivfpq_ivfflat_get_nprobe(const ivfpq_ivfflat_index* h) { return h ? h->nprobe : -1; }

int ivfpq_ivfflat_search(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I) {
  return with_handle(h, [&] {
    check_ivfflat_search(h, n, x, k, D, I);
    h->search_host(n, x, k, D, I, nullptr);
  });
}

int ivfpq_ivfflat_search_preassigned(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                     const float* Dq, float* D, int64_t* I) {
  return with_handle(h, [&] {
    (void)Dq;  // the scan computes whole distances (IVFFlatScanner ignores the coarse distance)
    check_ivfflat_search(h, n, x, k, D, I);
    require(n == 0 || Iq, "null Iq");
    for (int64_t i = 0; i < n * h->nprobe; i++) require(Iq[i] < h->nlist, "list id out of range in Iq");
    h->search_host(n, x, k, D, I, Iq);
  });
}

int ivfpq_ivfflat_search_device(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I,
                                void* stream) {
  return with_handle(h, [&] {
    check_ivfflat_search(h, n, x, k, D, I);
    h->search_dev(n, x, k, D, I, nullptr, (hipStream_t)stream);
  });
}

int ivfpq_ivfflat_search_preassigned_device(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k,
                                            const int64_t* Iq, const float* Dq, float* D, int64_t* I, void* stream) {
  return with_handle(h, [&] {
    (void)Dq;
    check_ivfflat_search(h, n, x, k, D, I);
    require(n == 0 || Iq, "null Iq");
    h->search_dev(n, x, k, D, I, n ? Iq : nullptr, (hipStream_t)stream);
  });
}

int64_t ivfpq_ivfflat_ntotal(const ivfpq_ivfflat_index* h) { return h ? h->ntotal : -1; }

int ivfpq_ivfflat_is_trained(const ivfpq_ivfflat_index* h) { return h && h->trained ? 1 : 0; }

int ivfpq_ivfflat_get_dims(const ivfpq_ivfflat_index* h, int* d, int* nlist, int* metric) {
  return guarded([&] {
    check_handle(h);
    if (d) *d = h->d;
    if (nlist) *nlist = h->nlist;
    if (metric) *metric = h->metric;
  });
}

int ivfpq_ivfflat_get_centroids(const ivfpq_ivfflat_index* h, float* out) {
  return guarded([&] {
    check_handle(h);
    require(h->trained, "index is not trained");
    require(out != nullptr, "null output pointer");
    std::memcpy(out, h->centroids.data(), sizeof(float) * h->centroids.size());
  });
}

int ivfpq_ivfflat_get_list_sizes(ivfpq_ivfflat_index* h, int64_t* out) {
  return with_handle(h, [&] {
    require(out != nullptr, "null output pointer");
    h->flush_pending(h->stream);
    for (int l = 0; l < h->nlist; l++) out[l] = h->h_off[l + 1] - h->h_off[l];
  });
}

int ivfpq_ivfflat_get_list(ivfpq_ivfflat_index* h, int list, float* vectors, int64_t* ids) {
  return with_handle(h, [&] {
    require(list >= 0 && list < h->nlist, "list id out of range");
    h->flush_pending(h->stream);
    h->quiesce();
    const int64_t b = h->h_off[list], n = h->h_off[list + 1] - b;
    if (n == 0) return;
    if (vectors)
      HIPCHECK(hipMemcpyAsync(vectors, h->img.rows.as<float>() + b * h->d, h->row_bytes() * n, hipMemcpyDeviceToHost,
                              h->stream));
    if (ids)
      HIPCHECK(hipMemcpyAsync(ids, h->img.ids.as<int64_t>() + b, sizeof(int64_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  });
}

}  // extern "C"
