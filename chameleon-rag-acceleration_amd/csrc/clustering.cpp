// Stand-alone k-means (faiss.Kmeans / faiss.Clustering) behind the C-ABI of include/ivfpq.h.
// Lloyd iterations whose n d work stays on the GPU: the assignment is the flat index's fused
// scan at k = 1 over the centroids (flat_scan.h: no distance matrix), the update is
// km_update.h's ordered fp64 accumulation, the objective a fixed-order fp64 reduction.  Per
// iteration only the k counts come to the host; the k d centroids follow them only when an
// empty cluster has to be split or the centroids renormalised (spherical), through
// kmeans_split_empty / renorm_rows of kmeans.h -- the host functions every *_train uses, so
// the result is oracle.kmeans' bit for bit.
#include <cstring>
#include <vector>

#include "code_store.h"  // open_store
#include "flat_scan.h"
#include "ivfpq.h"
#include "kmeans.h"
#include "km_update.h"

using namespace chivf;

namespace {

constexpr size_t kClusResidentBytes = size_t(8) << 30;  // host rows kept in HBM across iterations up to this
constexpr size_t kClusStageBytes = size_t(1) << 30;     // a streamed pass' rows
constexpr int64_t kClusPassRows = int64_t(1) << 24;      // rows per pass (28 bytes of scratch per row)
constexpr uint64_t kRedoSeedStep = 15486557ull;          // redo r trains from seed + r * this

struct ClusRun {
  std::vector<float> cent;
  std::vector<double> obj;
  std::vector<int64_t> nsplit;
};

}  // namespace

struct ivfpq_clus : StreamOrder {
  int device = 0, d = 0, k = 0, metric = IVFPQ_METRIC_L2;
  bool spherical = false;
  int64_t pass_rows = 0;  // > 0: forced (ivfpq_clus_set_pass_rows)
  hipStream_t stream = nullptr;
  std::mutex mu;
  ClusRun best;
  bool trained = false;
  DevBuf d_xall, d_stage, d_xn, d_cent, d_cn, d_sum, d_cnt, d_obj, d_D, d_I, d_pass, d_perm;
  DevBuf p_tau, p_partD, p_partI, p_tmpD, p_tmpI;

  ~ivfpq_clus() {
    if (stream) (void)hipStreamDestroy(stream);
  }
  bool ip() const { return metric == IVFPQ_METRIC_INNER_PRODUCT; }

  // rows per pass of n rows: the forced size, or what keeps a pass' scratch and staging bounded
  int64_t pass_size(int64_t n, bool staged) const {
    int64_t rows = pass_rows > 0 ? pass_rows : kClusPassRows;
    if (staged && pass_rows == 0) rows = std::min<int64_t>(rows, (int64_t)(kClusStageBytes / (sizeof(float) * d)));
    return std::max<int64_t>(1, std::min(n, rows));
  }

  // the c rows xd (device) with norms xn against the current centroids -> d_D, d_I
  void assign(const float* xd, const float* xn, int64_t c, int64_t qc, const FlatScanPlan& pl, hipStream_t s) {
    for (int64_t q0 = 0; q0 < c; q0 += qc) {
      FlatScanArgs a;
      a.x = xd + q0 * d;
      a.xn = xn + q0;
      a.nq = std::min(qc, c - q0);
      a.d = d;
      a.base = d_cent.as<float>();
      a.bn = d_cn.as<float>();
      a.nb = k;
      a.k = 1;
      a.ip = ip();
      a.tau = p_tau.as<uint32_t>();
      a.partD = p_partD.as<float>();
      a.partI = p_partI.as<int64_t>();
      a.tmpD = p_tmpD.as<float>();
      a.tmpI = p_tmpI.as<int64_t>();
      a.D = d_D.as<float>() + q0;
      a.I = d_I.as<int64_t>() + q0;
      launch_flat_search(a, pl, s);
      HIPCHECK(hipGetLastError());
    }
  }

  // x_dev: the rows in HBM, or null with x_host; init: k d host floats or null; all device work on s
  void train(int64_t n, const float* x_host, const float* x_dev, int niter, int nredo, uint64_t seed,
             const float* init, hipStream_t s) {
    require(n >= k, "k-means: need at least as many training points as centroids (" + std::to_string(n) + " < " +
                        std::to_string(k) + ")");
    require(n < (int64_t)INT32_MAX, "k-means: at most 2^31 - 2 training points");
    quiesce();
    const size_t kd = (size_t)k * d;
    bool resident = x_dev != nullptr;
    if (!resident && pass_rows == 0 && sizeof(float) * (size_t)n * d <= kClusResidentBytes) {
      d_xall.ensure(sizeof(float) * (size_t)n * d);
      HIPCHECK(hipMemcpyAsync(d_xall.p, x_host, sizeof(float) * (size_t)n * d, hipMemcpyHostToDevice, s));
      x_dev = d_xall.as<float>();
      resident = true;
    }
    const int64_t P = pass_size(n, !resident);
    if (!resident) d_stage.ensure(sizeof(float) * (size_t)P * d);
    FlatScanPlan pl;
    const int64_t qc = flat_query_chunk(P, k, 1, 0, &pl);
    p_tau.ensure(sizeof(uint32_t) * qc);
    p_partD.ensure(sizeof(float) * (size_t)pl.S * qc);
    p_partI.ensure(sizeof(int64_t) * (size_t)pl.S * qc);
    const size_t tmp_lists = (size_t)std::max(1, pl.S / pl.fan);
    p_tmpD.ensure(sizeof(float) * tmp_lists * qc);
    p_tmpI.ensure(sizeof(int64_t) * tmp_lists * qc);
    d_xn.ensure(sizeof(float) * (size_t)n);
    d_D.ensure(sizeof(float) * (size_t)P);
    d_I.ensure(sizeof(int64_t) * (size_t)P);
    d_pass.ensure(km_pass_scratch_bytes(P, k, n % P));
    const KmPassScratch w = km_pass_scratch(d_pass.p, P, k, n % P);
    d_cent.ensure(sizeof(float) * kd);
    d_cn.ensure(sizeof(float) * (size_t)k);
    d_sum.ensure(sizeof(double) * kd);
    d_cnt.ensure(sizeof(int64_t) * (size_t)k);
    d_obj.ensure(sizeof(double) * (size_t)std::max(niter, 1));
    // |x_i|^2 once per training set: here for resident rows, in the first iteration's passes otherwise
    bool have_xn = false;
    if (resident) {
      launch_row_norms(x_dev, n, d, d_xn.as<float>(), s);
      HIPCHECK(hipGetLastError());
      have_xn = true;
    }
    std::vector<int64_t> cnt(k);
    bool have_best = false;
    for (int r = 0; r < nredo; r++) {
      ClusRun run;
      run.cent.resize(kd);
      run.obj.assign(niter, 0.0);
      run.nsplit.assign(niter, 0);
      if (init) {
        std::memcpy(run.cent.data(), init, sizeof(float) * kd);
      } else {
        const auto perm = rand_perm_prefix(n, k, seed + kRedoSeedStep * (uint64_t)r);
        if (x_host) {
          for (int c = 0; c < k; c++) std::memcpy(&run.cent[(size_t)c * d], x_host + perm[c] * d, sizeof(float) * d);
        } else {
          d_perm.ensure(sizeof(int64_t) * (size_t)k);
          HIPCHECK(hipMemcpyAsync(d_perm.p, perm.data(), sizeof(int64_t) * (size_t)k, hipMemcpyHostToDevice, s));
          launch_km_gather_rows(x_dev, d, d_perm.as<int64_t>(), k, d_cent.as<float>(), s);
          HIPCHECK(hipGetLastError());
          HIPCHECK(hipMemcpyAsync(run.cent.data(), d_cent.p, sizeof(float) * kd, hipMemcpyDeviceToHost, s));
          HIPCHECK(hipStreamSynchronize(s));  // (perm is read until here)
        }
      }
      if (spherical) renorm_rows(run.cent.data(), k, d);  // Faiss post_process_centroids
      HIPCHECK(hipMemcpyAsync(d_cent.p, run.cent.data(), sizeof(float) * kd, hipMemcpyHostToDevice, s));
      HIPCHECK(hipMemsetAsync(d_obj.p, 0, sizeof(double) * (size_t)std::max(niter, 1), s));
      bool host_current = true;  // run.cent holds what d_cent holds
      for (int it = 0; it < niter; it++) {
        launch_row_norms(d_cent.as<float>(), k, d, d_cn.as<float>(), s);
        HIPCHECK(hipMemsetAsync(d_sum.p, 0, sizeof(double) * kd, s));
        HIPCHECK(hipMemsetAsync(d_cnt.p, 0, sizeof(int64_t) * (size_t)k, s));
        for (int64_t r0 = 0; r0 < n; r0 += P) {  // ascending: a later pass continues the chains
          const int64_t c = std::min(P, n - r0);
          const float* xd;
          if (resident) {
            xd = x_dev + r0 * d;
          } else {
            HIPCHECK(hipMemcpyAsync(d_stage.p, x_host + r0 * d, sizeof(float) * (size_t)c * d, hipMemcpyHostToDevice, s));
            xd = d_stage.as<float>();
          }
          float* xn = d_xn.as<float>() + r0;
          if (!have_xn) launch_row_norms(xd, c, d, xn, s);
          assign(xd, xn, c, qc, pl, s);
          HIPCHECK(launch_km_pass(xd, c, d, k, d_I.as<int64_t>(), d_D.as<float>(), w, d_sum.as<double>(),
                                  d_cnt.as<int64_t>(), d_obj.as<double>() + it, s));
        }
        have_xn = true;
        launch_km_mean(d_sum.as<double>(), d_cnt.as<int64_t>(), k, d, d_cent.as<float>(), s);
        HIPCHECK(hipGetLastError());
        HIPCHECK(hipMemcpyAsync(cnt.data(), d_cnt.p, sizeof(int64_t) * (size_t)k, hipMemcpyDeviceToHost, s));
        HIPCHECK(hipStreamSynchronize(s));
        host_current = false;
        bool empty = false;
        for (int c = 0; c < k && !empty; c++) empty = cnt[c] == 0;
        if (empty || spherical) {  // finalise on the host: k d numbers
          HIPCHECK(hipMemcpyAsync(run.cent.data(), d_cent.p, sizeof(float) * kd, hipMemcpyDeviceToHost, s));
          HIPCHECK(hipStreamSynchronize(s));
          if (empty) run.nsplit[it] = kmeans_split_empty(run.cent.data(), cnt.data(), k, d);
          if (spherical) renorm_rows(run.cent.data(), k, d);
          HIPCHECK(hipMemcpyAsync(d_cent.p, run.cent.data(), sizeof(float) * kd, hipMemcpyHostToDevice, s));
          host_current = true;
        }
      }
      if (!host_current) HIPCHECK(hipMemcpyAsync(run.cent.data(), d_cent.p, sizeof(float) * kd, hipMemcpyDeviceToHost, s));
      if (niter > 0)
        HIPCHECK(hipMemcpyAsync(run.obj.data(), d_obj.p, sizeof(double) * (size_t)niter, hipMemcpyDeviceToHost, s));
      HIPCHECK(hipStreamSynchronize(s));
      // the best final objective: smallest for L2, largest for inner product; ties keep the earlier run
      bool better = !have_best;
      if (have_best && niter > 0) {
        const double a = run.obj[niter - 1], b = best.obj[niter - 1];
        better = ip() ? a > b : a < b;
      }
      if (better) best = std::move(run);
      have_best = true;
    }
    trained = true;
    d_xall.release();
    d_stage.release();
  }
};

extern "C" {

int ivfpq_clus_create(int d, int k, int metric, int spherical, int device, ivfpq_clus** out) {
  return guarded([&] {
    require(out != nullptr, "null output pointer");
    require(d >= 1, "Clustering: d must be at least 1 (d = " + std::to_string(d) + ")");
    require(k >= 1, "Clustering: k must be at least 1 (k = " + std::to_string(k) + ")");
    require(metric == IVFPQ_METRIC_L2 || metric == IVFPQ_METRIC_INNER_PRODUCT,
            "Clustering: unknown metric " + std::to_string(metric));
    const bool ip = metric == IVFPQ_METRIC_INNER_PRODUCT;
    require(ip == (spherical != 0),
            std::string("Clustering: ") + (ip ? "inner product" : "L2") + " with spherical = " +
                (spherical ? "true" : "false") +
                " is not supported (the pairs are L2 with spherical = false, inner product with spherical = true)");
    auto h = std::make_unique<ivfpq_clus>();
    h->d = d;
    h->k = k;
    h->metric = metric;
    h->spherical = spherical != 0;
    open_store(std::move(h), device, out);
  });
}

int ivfpq_clus_free(ivfpq_clus* h) { return free_handle(h); }

static void check_train_args(int64_t n, const float* x, int niter, int nredo) {
  require(niter >= 0, "Clustering: niter must be at least 0 (niter = " + std::to_string(niter) + ")");
  require(nredo >= 1, "Clustering: nredo must be at least 1 (nredo = " + std::to_string(nredo) + ")");
  require(x != nullptr && n > 0, "empty training set");
}

int ivfpq_clus_train(ivfpq_clus* h, int64_t n, const float* x, int niter, int nredo, uint64_t seed,
                     const float* init) {
  return guarded([&] {
    check_train_args(n, x, niter, nredo);  // (before the handle, as the searches check theirs)
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->train(n, x, nullptr, niter, nredo, seed, init, h->stream);
  });
}

int ivfpq_clus_train_device(ivfpq_clus* h, int64_t n, const float* x, int niter, int nredo, uint64_t seed,
                            const float* init, void* stream) {
  return guarded([&] {
    check_train_args(n, x, niter, nredo);  // (before the handle, as the searches check theirs)
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    DeviceGuard g(h->device);
    h->train(n, nullptr, x, niter, nredo, seed, init, (hipStream_t)stream);
  });
}

int ivfpq_clus_get_centroids(ivfpq_clus* h, float* out) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    require(h->trained, "Clustering: not trained");
    require(out != nullptr, "null output pointer");
    std::memcpy(out, h->best.cent.data(), sizeof(float) * h->best.cent.size());
  });
}

int ivfpq_clus_get_stats(ivfpq_clus* h, int* niter, double* obj, int64_t* nsplit) {
  return guarded([&] {
    check_handle(h);
    std::lock_guard<std::mutex> lk(h->mu);
    require(h->trained, "Clustering: not trained");
    if (niter) *niter = (int)h->best.obj.size();
    if (obj) std::memcpy(obj, h->best.obj.data(), sizeof(double) * h->best.obj.size());
    if (nsplit) std::memcpy(nsplit, h->best.nsplit.data(), sizeof(int64_t) * h->best.nsplit.size());
  });
}

int ivfpq_clus_set_pass_rows(ivfpq_clus* h, int64_t rows) {
  return guarded([&] {
    check_handle(h);
    require(rows >= 0, "negative pass size");
    std::lock_guard<std::mutex> lk(h->mu);
    h->pass_rows = rows;
  });
}

int ivfpq_clus_rand_perm_prefix(int64_t n, int64_t k, uint64_t seed, int64_t* out) {
  return guarded([&] {
    require(n >= 0 && k >= 0 && k <= n, "rand_perm_prefix: need 0 <= k <= n");
    require(k == 0 || out != nullptr, "null output pointer");
    const auto p = rand_perm_prefix(n, k, seed);
    if (k) std::memcpy(out, p.data(), sizeof(int64_t) * (size_t)k);
  });
}

}  // extern "C"
