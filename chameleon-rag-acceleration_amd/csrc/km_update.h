// Launchers of the resident k-means update (km_update.hip) behind Kmeans / Clustering
// (clustering.cpp): one pass of rows, already assigned by launch_flat_search at k = 1, is
// ordered by cluster and added into the clusters' fp64 sums.  Every sum[c][t] is ONE chain
// of fp64 additions over the cluster's rows in ascending row order -- kmeans_update's order
// (kmeans.h), so the sums are the host's bit for bit; passes taken in ascending row order
// continue the same chains.  No floating-point atomics: two runs give the same bits.
// All launchers are asynchronous on `stream` and allocate nothing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace chivf {

constexpr int kKmBatch = 16;       // rows a lane loads before it adds them, in order
constexpr int kKmObjBlock = 4096;  // keys per workgroup partial of the objective (256 threads x 16)

// The scratch of one pass of `rows` rows into k clusters (and of a shorter last pass of
// tail_rows, whose sort states its own need), cut from one allocation.
struct KmPassScratch {
  uint32_t *key = nullptr, *key2 = nullptr;    // [rows] the rows' clusters, before / after the sort
  uint32_t *row = nullptr, *row2 = nullptr;    // [rows] the rows' positions in the pass
  int64_t* off = nullptr;                      // [k + 1] the clusters' offsets into row2
  uint32_t *len = nullptr, *len2 = nullptr;    // [k] the clusters' row counts in this pass
  uint32_t *clus = nullptr, *order = nullptr;  // [k] the clusters, longest first in `order`
  double* part = nullptr;                      // [ceil(rows / kKmObjBlock)] objective partials
  void* sort_tmp = nullptr;
  size_t sort_bytes = 0;
};
size_t km_pass_scratch_bytes(int64_t rows, int k, int64_t tail_rows);
KmPassScratch km_pass_scratch(void* base, int64_t rows, int k, int64_t tail_rows);

// One pass: assign [rows] (launch_flat_search's labels) and D [rows] (its keys) of the rows
// x [rows][d]; sum [k][d] and cnt [k] take the pass' rows, *obj its sum of (double)D[i]
// (per-workgroup partials in a fixed order, then one final workgroup).  rows < 2^31.
hipError_t launch_km_pass(const float* x, int64_t rows, int d, int k, const int64_t* assign, const float* D,
                          const KmPassScratch& w, double* sum, int64_t* cnt, double* obj, hipStream_t s);

// cent[c][t] = (float)(sum[c][t] / (double)cnt[c]) for the clusters with cnt[c] > 0 (the
// others keep their centroid: kmeans_update's first loop)
void launch_km_mean(const double* sum, const int64_t* cnt, int k, int d, float* cent, hipStream_t s);

// out[c] = x[idx[c]] (the initial centroids of rows resident in HBM)
void launch_km_gather_rows(const float* x, int d, const int64_t* idx, int k, float* out, hipStream_t s);

}  // namespace chivf
