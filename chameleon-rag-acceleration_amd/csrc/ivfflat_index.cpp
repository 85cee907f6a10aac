// IVF-Flat (IndexIVFFlat) behind the C-ABI of include/ivfpq.h.
// faiss.IndexIVFFlat: IVF-PQ's coarse quantizer (k-means, matrix-core keys,
// top-nprobe selection) over inverted lists of the raw fp32 vectors, scanned by
// ivf_flat.hip.  The vectors live only in the device image {list_off, vectors, ids},
// every list sorted by label; adds wait in a pending set on the device and are merged
// with the image kernels of ivfpq_build.h at code size 4 d.  The handle -- image, pending
// set, workspaces, the search around the scan and the entry points that IVF over
// scalar-quantizer codes has too -- is ivf_lists.h's IvfLists; this file keeps the
// fp32 rows: their add, the scan's launch, create, train and the entry points' names.
#include <memory>
#include <vector>

#include "ivf_flat.h"
#include "ivf_lists.h"
#include "ivfpq.h"
#include "kmeans.h"

using namespace chivf;

struct ivfpq_ivfflat_index : IvfLists {
  IvfFlatPlan plan(int k, int64_t slots) const override { return ivfflat_plan(k, slots); }
  void launch_chunk(const IvfFlatArgs& f, const IvfFlatPlan& pl, const float*, hipStream_t s) override {
    launch_ivfflat_search(f, pl, s);  // (IVFFlatScanner computes whole distances: no coarse value is read)
  }

  // n vectors (host or device) into the pending set: copied behind it, then assigned
  // there by the search's coarse kernels (top-1), as IVF-PQ's add_dev assigns.
  void add_dev(int64_t n, const float* x, bool x_on_device, const int64_t* ids, bool ids_on_device, hipStream_t s) {
    if (n <= 0) return;
    reserve_pending(n, s);
    const int64_t rows = chunk_rows(n, false);
    float* xd = q.rows.as<float>() + q.n * d;
    int64_t* lists = q.lists.as<int64_t>() + q.n;
    HIPCHECK(hipMemcpyAsync(xd, x, row_bytes() * n, x_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
    w_D.ensure(sizeof(float) * rows);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      cq.launch(cw, xd + r0 * d, c, 1, w_D.as<float>(), lists + r0, s);
      HIPCHECK(hipGetLastError());
    }
    pending_ids(n, ids, ids_on_device, s);
    commit_pending(n, s);
  }
};

extern "C" {

int ivfpq_ivfflat_create(int d, int nlist, int metric, int device, ivfpq_ivfflat_index** out) {
  return guarded([&] {
    check_ivf_create("IndexIVFFlat", out, d, nlist);
    check_ivf_device(metric, device);
    DeviceGuard g(device);
    auto h = std::make_unique<ivfpq_ivfflat_index>();
    h->open("IndexIVFFlat", d, nlist, metric, device, sizeof(float) * (size_t)d, 0);
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
    require(h->trained(), "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, false, ids, false, h->stream);
  });
}

int ivfpq_ivfflat_add_device(ivfpq_ivfflat_index* h, int64_t n, const float* x, const int64_t* ids, void* stream) {
  return with_handle(h, [&] {
    require(h->trained(), "index is not trained");
    if (n <= 0) return;
    require(x != nullptr, "null x");
    h->add_dev(n, x, true, ids, true, stream ? (hipStream_t)stream : h->stream);
  });
}

int ivfpq_ivfflat_reset(ivfpq_ivfflat_index* h) { return ivf_reset(h); }

int ivfpq_ivfflat_set_nprobe(ivfpq_ivfflat_index* h, int nprobe) { return ivf_set_nprobe(h, nprobe); }

int ivfpq_ivfflat_get_nprobe(const ivfpq_ivfflat_index* h) { return ivf_get_nprobe(h); }

int ivfpq_ivfflat_search(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I) {
  return ivf_search(h, n, x, k, D, I);
}

// (Dq is not read: the scan computes whole distances, as IVFFlatScanner ignores the coarse distance)
int ivfpq_ivfflat_search_preassigned(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                     const float*, float* D, int64_t* I) {
  return ivf_search_preassigned(h, n, x, k, Iq, nullptr, D, I);
}

int ivfpq_ivfflat_search_device(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I,
                                void* stream) {
  return ivf_search_device(h, n, x, k, D, I, stream);
}

int ivfpq_ivfflat_search_preassigned_device(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k,
                                            const int64_t* Iq, const float*, float* D, int64_t* I, void* stream) {
  return ivf_search_preassigned_device(h, n, x, k, Iq, nullptr, D, I, stream);
}

int64_t ivfpq_ivfflat_ntotal(const ivfpq_ivfflat_index* h) { return ivf_ntotal(h); }

int ivfpq_ivfflat_is_trained(const ivfpq_ivfflat_index* h) { return h && h->trained() ? 1 : 0; }

int ivfpq_ivfflat_get_dims(const ivfpq_ivfflat_index* h, int* d, int* nlist, int* metric) {
  return guarded([&] {
    check_handle(h);
    if (d) *d = h->d;
    if (nlist) *nlist = h->nlist;
    if (metric) *metric = h->metric;
  });
}

int ivfpq_ivfflat_get_centroids(const ivfpq_ivfflat_index* h, float* out) { return ivf_get_centroids(h, out); }

int ivfpq_ivfflat_get_list_sizes(ivfpq_ivfflat_index* h, int64_t* out) { return ivf_get_list_sizes(h, out); }

int ivfpq_ivfflat_get_list(ivfpq_ivfflat_index* h, int list, float* vectors, int64_t* ids) {
  return ivf_get_list(h, list, vectors, ids);
}

// ---- how IvfLists cuts a batch (IndexIVFFlat and IndexIVFScalarQuantizer): host arithmetic ----
int ivfpq_ivf_get_plan(int k, int64_t slots, int* S, int* fan) {
  return guarded([&] {
    require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
    require(slots >= 0 && slots < (int64_t)INT32_MAX / kIvfFlatWaves / 2, "slots out of range");
    const IvfFlatPlan pl = ivfflat_plan(k, slots);  // (ivfsq_plan differs in G alone)
    if (S) *S = pl.S;
    if (fan) *fan = pl.fan;
  });
}

int ivfpq_ivf_get_query_chunk(int64_t nq, int nlist, int entry_bytes, int S, int k, int nprobe, int d,
                              int resid_queries, int64_t* query_chunk) {
  return guarded([&] {
    require(k >= 1 && k <= kMaxK, "k must be in [1, " + std::to_string(kMaxK) + "]");
    require(nq >= 0 && nlist >= 1 && entry_bytes >= 1 && S >= 1 && nprobe >= 1 && d >= 1, "shape out of range");
    if (query_chunk) *query_chunk = ivf_query_chunk(nq, nlist, (size_t)entry_bytes, S, k, nprobe, d, resid_queries != 0);
  });
}

int ivfpq_ivf_get_pass_rows(int64_t n, int nlist, int d, int staged, int64_t* rows) {
  return guarded([&] {
    require(n >= 0 && nlist >= 1 && d >= 1, "shape out of range");
    if (rows) *rows = ivf_pass_rows(n, nlist, d, staged != 0);
  });
}

}  // extern "C"
