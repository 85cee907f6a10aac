// The handle of an IVF index over fixed-size rows, as IndexIVFFlat (rows = the fp32 vectors,
// ivfflat_index.cpp) and IndexIVFScalarQuantizer (rows = fp16 / 8-bit codes, ivfsq_index.cpp)
// keep it: IVF-PQ's coarse quantizer, the device image {list_off, rows, ids} with every list
// sorted by label, the pending set of device-side adds and its merge, the planning workspace of
// the list-major scans (ivf_flat.h) and the search around them, and the C-ABI entry points that
// are the same for both.  The row type adds its plan, its bytes in the chunk bound, its own
// workspaces and the launch of one chunk.  Device calls on different streams are ordered one
// after the other (one workspace per handle).  Host code only.
#pragma once
#include <cstring>
#include <functional>
#include <vector>

#include "coarse_quantizer.h"
#include "ivf_flat.h"
#include "ivfpq.h"
#include "list_image.h"

namespace chivf {

struct IvfLists : StreamOrder {
  const char* name = "";  // Faiss's name of the index, for messages
  int d = 0, nlist = 0, metric = IVFPQ_METRIC_L2, device = 0;
  int nprobe = 1;
  bool cent_trained = false;
  std::vector<float> centroids;  // [nlist][d]
  CoarseQuantizer cq;
  CoarseScratch cw;
  int64_t ntotal = 0, next_id = 0;
  int64_t img_n = 0;  // rows in the image (ntotal = img_n + q.n)
  ListImage img;
  std::vector<int64_t> h_off;      // the image's list offsets
  std::vector<int64_t> range_top;  // range_top[p] = row ranges of the p longest lists (the slot bound)
  PendingSet q;                    // pending adds: list numbers, labels, rows
  DevBuf w_D, w_x, h_D, h_I, h_Iq, h_Dq;  // add scratch; staging of the host entry points
  DevBuf w_lists, w_dis, p_cnt, p_bucket, p_items, p_used, p_tau, p_partD, p_partI, p_tmpD, p_tmpI;
  hipStream_t stream = nullptr;
  std::mutex mu;

  virtual ~IvfLists() {
    if (stream) (void)hipStreamDestroy(stream);
  }
  bool ip() const { return metric == IVFPQ_METRIC_INNER_PRODUCT; }
  size_t row_bytes() const { return q.row_bytes; }

  // ---- what the row type contributes -------------------------------------------
  virtual bool trained() const { return cent_trained; }
  // the scan's plan for k and a slot bound
  virtual IvfFlatPlan plan(int k, int64_t slots) const = 0;
  // bytes per [query][list] entry of a chunk: the coarse keys and the buckets, and what the row type adds
  virtual size_t entry_bytes() const { return 8; }
  // whether a chunk keeps its [c][np][d] residual queries (they bound the chunk: ivf_query_chunk)
  virtual bool resid_queries() const { return false; }
  // The row type's own workspaces for chunks of at most qc queries with np probes each, before
  // the first chunk.  zero_coarse: the probes are preassigned without their coarse values.
  virtual void prepare_chunks(int64_t qc, int np, bool zero_coarse, hipStream_t s) {
    (void)qc, (void)np, (void)zero_coarse, (void)s;
  }
  // plan + scan + merge of one chunk; cdis: [f.nq][f.nprobe] coarse values of the probes (null:
  // preassigned without them)
  virtual void launch_chunk(const IvfFlatArgs& f, const IvfFlatPlan& pl, const float* cdis, hipStream_t s) = 0;

  // ---- create / train ----------------------------------------------------------
  // dimensions, stream and an empty image (row_bytes: of a stored row; image_slack: PendingSet's)
  void open(const char* index_name, int d_, int nlist_, int metric_, int device_, size_t row_bytes_,
            size_t image_slack) {
    name = index_name;
    d = cq.d = d_;
    nlist = cq.nlist = nlist_;
    metric = cq.metric = metric_;
    device = device_;
    q.row_bytes = row_bytes_;
    q.image_slack = image_slack;
    HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    create();
    clear_image();
  }

  void upload_centroids() {
    quiesce();
    cq.upload(centroids.data(), stream);
    cent_trained = true;
  }

  // ---- the image and the pending set -------------------------------------------
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

  // rows per pass of add and train (ivf_pass_rows; staged: the pass has a [rows][d] fp32 staging buffer)
  int64_t chunk_rows(int64_t n, bool staged) const { return ivf_pass_rows(n, nlist, d, staged); }

  // An add of n rows: room behind the pending set (reserve), then the caller writes the rows
  // and their lists there on s, then the labels (ids) and the commit.  The pending set is
  // merged into the image before the lists are next read, or once it is as large as the image
  // (and at least kChunkBytes), so that a sequence of adds moves every row O(1) times.
  void reserve_pending(int64_t n, hipStream_t s) {
    require(ntotal + n < (int64_t)INT32_MAX, std::string(name) + " holds fewer than 2^31 - 1 vectors");
    order_after(s);
    quiesce();
    q.reserve(q.n + n, s);
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
  void commit_pending(int64_t n, hipStream_t s) {
    HIPCHECK(hipStreamSynchronize(s));
    q.n += n;
    ntotal += n;
    if (q.n >= std::max<int64_t>(img_n, (int64_t)(kChunkBytes / row_bytes()))) flush_pending(s);
  }

  // the pending rows merged into the image (merge_pending at the row's size; the new image is
  // allocated with q.image_slack behind its last row)
  void flush_pending(hipStream_t s) {
    if (q.n == 0) return;
    quiesce();
    set_offsets(merge_pending(q, img, nlist, 0, nlist, h_off.data(), q.n,
                              "pending merge: a vector was assigned to no list", s));
    img_n = h_off[nlist];
    require(img_n == ntotal, "pending merge: image size disagrees with ntotal");
  }

  // ---- search ------------------------------------------------------------------
  // The search on device pointers, on stream s.  Iq non-null = preassigned probes [n][nprobe]
  // (the handle's nprobe, as ivfpq_search_preassigned) with their coarse values Dq (nullable;
  // read where the row type's distances include them).
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
    const IvfFlatPlan pl = plan(k, range_top[std::min(np, nlist)]);
    const int64_t qc = ivf_query_chunk(n, nlist, entry_bytes(), pl.S, k, np, d, resid_queries());
    prepare_chunks(qc, np, Iq && !Dq, s);
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
      a.vecs = img.rows.as<float>();  // (read by the fp32 scan alone)
      a.ids = img.ids.as<int64_t>();
      a.list_off = img.off.as<int64_t>();
      a.nlist = nlist;
      const float* cdis = nullptr;
      if (Iq) {
        a.probes = Iq + q0 * np;
        if (Dq) cdis = Dq + q0 * np;
      } else {
        cq.launch(cw, xq, c, np, w_dis.as<float>(), w_lists.as<int64_t>(), s);
        a.probes = w_lists.as<int64_t>();
        cdis = w_dis.as<float>();
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
      launch_chunk(a, pl, cdis, s);
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

// ---- the C-ABI entry points both indexes have --------------------------------------
// the arguments of ivfpq_create that both take, in its words
inline void check_ivf_create(const char* name, const void* out, int d, int nlist) {
  require(out != nullptr, "null output pointer");
  require(d >= 4 && d <= 2048 && d % 4 == 0,
          std::string(name) + ": d must be a multiple of 4 in [4, 2048] (d = " + std::to_string(d) + ")");
  require(nlist >= 1, "nlist must be >= 1");
}
inline void check_ivf_device(int metric, int device) {
  require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT, "unknown metric");
  int ndev = 0;
  HIPCHECK(hipGetDeviceCount(&ndev));
  require(device >= 0 && device < ndev, "device ordinal out of range");
}

// the search arguments, in the words of ivfpq_search
inline void check_ivf_search(const IvfLists* h, int64_t n, const void* x, int k, const void* D, const void* I) {
  check_search_args(h->trained(), n, k);
  require(n == 0 || (x && D && I), "null buffer");
}

inline int ivf_reset(IvfLists* h) {
  return with_handle(h, [&] { h->clear_image(); });
}

inline int ivf_set_nprobe(IvfLists* h, int nprobe) {
  return guarded([&] {
    check_handle(h);
    require(nprobe >= 1 && nprobe <= kMaxK, "nprobe must be in [1, " + std::to_string(kMaxK) + "]");
    h->nprobe = nprobe;
  });
}

inline int ivf_get_nprobe(const IvfLists* h) { return h ? h->nprobe : -1; }

inline int64_t ivf_ntotal(const IvfLists* h) { return h ? h->ntotal : -1; }

inline int ivf_get_centroids(const IvfLists* h, float* out) {
  return guarded([&] {
    check_handle(h);
    require(h->cent_trained, "index is not trained");
    require(out != nullptr, "null output pointer");
    std::memcpy(out, h->centroids.data(), sizeof(float) * h->centroids.size());
  });
}

inline int ivf_get_list_sizes(IvfLists* h, int64_t* out) {
  return with_handle(h, [&] {
    require(out != nullptr, "null output pointer");
    h->flush_pending(h->stream);
    for (int l = 0; l < h->nlist; l++) out[l] = h->h_off[l + 1] - h->h_off[l];
  });
}

inline int ivf_search(IvfLists* h, int64_t n, const float* x, int k, float* D, int64_t* I) {
  return with_handle(h, [&] {
    check_ivf_search(h, n, x, k, D, I);
    h->search_host(n, x, k, D, I, nullptr, nullptr);
  });
}

inline int ivf_search_preassigned(IvfLists* h, int64_t n, const float* x, int k, const int64_t* Iq, const float* Dq,
                                  float* D, int64_t* I) {
  return with_handle(h, [&] {
    check_ivf_search(h, n, x, k, D, I);
    require(n == 0 || Iq, "null Iq");
    for (int64_t i = 0; i < n * h->nprobe; i++) require(Iq[i] < h->nlist, "list id out of range in Iq");
    h->search_host(n, x, k, D, I, Iq, Dq);
  });
}

inline int ivf_search_device(IvfLists* h, int64_t n, const float* x, int k, float* D, int64_t* I, void* stream) {
  return with_handle(h, [&] {
    check_ivf_search(h, n, x, k, D, I);
    h->search_dev(n, x, k, D, I, nullptr, nullptr, (hipStream_t)stream);
  });
}

inline int ivf_search_preassigned_device(IvfLists* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                         const float* Dq, float* D, int64_t* I, void* stream) {
  return with_handle(h, [&] {
    check_ivf_search(h, n, x, k, D, I);
    require(n == 0 || Iq, "null Iq");
    h->search_dev(n, x, k, D, I, n ? Iq : nullptr, Dq, (hipStream_t)stream);
  });
}

// one list of the image to the host: its rows (row_bytes each) and labels, either nullable
inline int ivf_get_list(IvfLists* h, int list, void* rows, int64_t* ids) {
  return with_handle(h, [&] {
    require(list >= 0 && list < h->nlist, "list id out of range");
    h->flush_pending(h->stream);
    h->quiesce();
    const int64_t b = h->h_off[list], n = h->h_off[list + 1] - b;
    if (n == 0) return;
    if (rows)
      HIPCHECK(hipMemcpyAsync(rows, h->img.rows.as<uint8_t>() + b * h->row_bytes(), h->row_bytes() * n,
                              hipMemcpyDeviceToHost, h->stream));
    if (ids)
      HIPCHECK(hipMemcpyAsync(ids, h->img.ids.as<int64_t>() + b, sizeof(int64_t) * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
  });
}

}  // namespace chivf
