// GPU k-means of the *_train entry points: assignment on the GPU, the centroid update (a
// per-cluster double-precision mean) on the host.  Same generator and update rule as the
// oracle (oracle/ivfpq_oracle.c, or_rand_perm_prefix / or_kmeans_update / or_renorm_rows)
// so GPU-trained and oracle-trained indexes are identical for identical input.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "host_common.h"

namespace chivf {

inline uint64_t splitmix(uint64_t* s) {
  uint64_t z = (*s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

inline std::vector<int64_t> rand_perm_prefix(int64_t n, int64_t k, uint64_t seed) {
  std::vector<int64_t> p(n), out(k);
  for (int64_t i = 0; i < n; i++) p[i] = i;
  uint64_t s = seed;
  for (int64_t i = 0; i < k; i++) {
    int64_t j = i + (int64_t)(splitmix(&s) % (uint64_t)(n - i));
    std::swap(p[i], p[j]);
    out[i] = p[i];
  }
  return out;
}

// Spherical k-means step (Faiss Clustering with spherical = true, which IndexIVF
// sets for METRIC_INNER_PRODUCT; fvec_renorm_L2): every centroid scaled to unit
// L2 norm.
inline void renorm_rows(float* x, int64_t n, int d) {
  for (int64_t i = 0; i < n; i++) {
    float* xi = x + i * d;
    float nr = 0.f;
    for (int t = 0; t < d; t++) nr += xi[t] * xi[t];
    if (nr > 0.f) {
      const float inv = (float)(1.0 / (double)sqrtf(nr));
      for (int t = 0; t < d; t++) xi[t] *= inv;
    }
  }
}

// The second loop of a k-means update (Faiss split_clusters' rule, the oracle's order): every
// empty cluster, in ascending order, takes the largest cluster's centroid, the two perturbed
// by +-1/1024 in alternating dimensions, and half its count.  Returns the clusters split.
inline int64_t kmeans_split_empty(float* cent, int64_t* cnt, int k, int d) {
  const float eps = 1.0f / 1024.0f;
  int64_t nsplit = 0;
  for (int c = 0; c < k; c++) {
    if (cnt[c] != 0) continue;
    nsplit++;
    int big = 0;
    for (int j = 1; j < k; j++)
      if (cnt[j] > cnt[big]) big = j;
    for (int t = 0; t < d; t++) {
      const float v = cent[(size_t)big * d + t];
      if (t % 2 == 0) {
        cent[(size_t)c * d + t] = v * (1.0f + eps);
        cent[(size_t)big * d + t] = v * (1.0f - eps);
      } else {
        cent[(size_t)c * d + t] = v * (1.0f - eps);
        cent[(size_t)big * d + t] = v * (1.0f + eps);
      }
    }
    cnt[c] = cnt[big] / 2;
    cnt[big] -= cnt[c];
  }
  return nsplit;
}

inline void kmeans_update(const float* x, int64_t n, int d, int k, const int64_t* assign, float* cent) {
  std::vector<double> sum((size_t)k * d, 0.0);
  std::vector<int64_t> cnt(k, 0);
  for (int64_t i = 0; i < n; i++) {
    const int64_t c = assign[i];
    cnt[c]++;
    double* s = &sum[(size_t)c * d];
    const float* xi = x + i * d;
    for (int t = 0; t < d; t++) s[t] += (double)xi[t];
  }
  for (int c = 0; c < k; c++)
    if (cnt[c] > 0)
      for (int t = 0; t < d; t++) cent[(size_t)c * d + t] = (float)(sum[(size_t)c * d + t] / (double)cnt[c]);
  kmeans_split_empty(cent, cnt.data(), k, d);
}

// One training run's scratch, on the stream it is given; made and released by the
// *_train call that uses it.
struct KMeans {
  hipStream_t stream;
  DevBuf w_x, w_xn, w_dist, w_D, w_I, w_cent, w_cn;

  explicit KMeans(hipStream_t s) : stream(s) {}

  // Row-wise top-1 of x [n][dd] against the k centroids cent (host): writes the
  // assignments (host) of all rows.  x_dev: the rows' device copy, when they are resident.
  // ip_assign: assign to the largest inner product (the IndexFlatIP quantizer of an IP index)
  void assign_top1(const float* x_host, int64_t n, int dd, const float* cent, int k, int64_t* assign_host,
                   const float* x_dev = nullptr, bool ip_assign = false) {
    w_cent.ensure(sizeof(float) * k * dd);
    w_cn.ensure(sizeof(float) * k);
    HIPCHECK(hipMemcpyAsync(w_cent.p, cent, sizeof(float) * k * dd, hipMemcpyHostToDevice, stream));
    launch_row_norms(w_cent.as<float>(), k, dd, w_cn.as<float>(), stream);
    const int64_t rows = kmeans_assign_rows(n, k);
    w_xn.ensure(sizeof(float) * rows);
    w_dist.ensure(sizeof(float) * rows * k);
    w_D.ensure(sizeof(float) * rows);
    w_I.ensure(sizeof(int64_t) * rows);
    if (!x_dev) w_x.ensure(sizeof(float) * rows * dd);
    for (int64_t r0 = 0; r0 < n; r0 += rows) {
      const int64_t c = std::min(rows, n - r0);
      const float* xd;
      if (x_dev) {
        xd = x_dev + r0 * dd;
      } else {
        HIPCHECK(hipMemcpyAsync(w_x.p, x_host + r0 * dd, sizeof(float) * c * dd, hipMemcpyHostToDevice, stream));
        xd = w_x.as<float>();
      }
      if (!ip_assign) launch_row_norms(xd, c, dd, w_xn.as<float>(), stream);
      launch_l2_dist(xd, w_xn.as<float>(), c, w_cent.as<float>(), w_cn.as<float>(), k, dd, w_dist.as<float>(), stream,
                     ip_assign);
      launch_select_rows(w_dist.as<float>(), c, k, 1, w_D.as<float>(), w_I.as<int64_t>(), stream);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipMemcpyAsync(assign_host + r0, w_I.p, sizeof(int64_t) * c, hipMemcpyDeviceToHost, stream));
      HIPCHECK(hipStreamSynchronize(stream));
    }
  }

  void kmeans(const float* x, int64_t n, int dd, int k, int niter, uint64_t seed, float* cent,
              bool ip_assign = false) {
    require(n >= k, "k-means: need at least as many training points as centroids (" + std::to_string(n) + " < " +
                        std::to_string(k) + ")");
    const auto init = rand_perm_prefix(n, k, seed);
    for (int c = 0; c < k; c++) std::memcpy(cent + (size_t)c * dd, x + init[c] * dd, sizeof(float) * dd);
    if (ip_assign) renorm_rows(cent, k, dd);  // spherical: unit-norm centroids (Faiss post_process_centroids)
    // keep the whole training set resident when it fits the scratch bound
    DevBuf xall;
    const bool resident = (size_t)n * dd * 4 <= (size_t(2) << 30);
    if (resident) {
      xall.ensure(sizeof(float) * n * dd);
      HIPCHECK(hipMemcpyAsync(xall.p, x, sizeof(float) * n * dd, hipMemcpyHostToDevice, stream));
    }
    std::vector<int64_t> assign(n);
    for (int it = 0; it < niter; it++) {
      assign_top1(x, n, dd, cent, k, assign.data(), resident ? xall.as<float>() : nullptr, ip_assign);
      kmeans_update(x, n, dd, k, assign.data(), cent);
      if (ip_assign) renorm_rows(cent, k, dd);
    }
  }
};

}  // namespace chivf
