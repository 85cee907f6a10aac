// gfx950 (MI355X, CDNA4) kernels of the resident k-means update (Kmeans / Clustering).
//
// A pass of rows arrives assigned (launch_flat_search at k = 1: label a[i], key D[i]).
//   order:      one stable rocprim radix sort of (a[i], i) over key_bits(k) bits.  The rows go in
//               ascending, so every cluster's rows come out in ascending row order; the clusters'
//               offsets follow from the sorted keys (launch_list_offsets).
//   accumulate: k_km_accumulate, the hot kernel.  sum[c][t] += (double)x[i][t] over cluster c's
//               rows of the pass in ascending i, one fp64 chain per (c, t): kmeans_update's
//               order, so the sums are the host's bit for bit, and a later pass continues the
//               chain from the value this one stored.  One wave per (cluster, 64-dimension
//               slice), lanes as dimensions; below 64 dimensions a wave takes 64 / dpad clusters
//               (dpad: d rounded up to a power of two), so d = 8 still fills its lanes.  A lane
//               loads kKmBatch rows of its cluster at once (independent loads, the next batch's
//               row numbers fetched behind them) and then adds them in order.  The clusters are
//               handed out longest first (a second, descending sort of the k row counts): the
//               longest chain, which bounds the kernel, starts first and the short ones fill in
//               behind it.
//   objective:  obj += sum of (double)D[i]: every workgroup reduces kKmObjBlock keys in a fixed
//               order to one fp64 partial, one final workgroup reduces the partials.
// No floating-point atomics anywhere.  Compiled with -ffp-contract=off like the rest.
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "ivfpq_build.h"
#include "km_update.h"

namespace chivf {

namespace {

inline unsigned nblk(int64_t n, int t) { return (unsigned)std::max<int64_t>(1, (n + t - 1) / t); }

// sort keys of a pass: the row's cluster (k for a label outside [0, k): sorted behind every
// cluster and never read) and its position
__global__ __launch_bounds__(256) void k_km_keys(const int64_t* __restrict__ assign, int64_t n, int k,
                                                 uint32_t* __restrict__ key, uint32_t* __restrict__ row) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t a = assign[i];
  key[i] = (a >= 0 && a < k) ? (uint32_t)a : (uint32_t)k;
  row[i] = (uint32_t)i;
}

__global__ __launch_bounds__(256) void k_km_lens(const int64_t* __restrict__ off, int k, uint32_t* __restrict__ len,
                                                 uint32_t* __restrict__ clus) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= k) return;
  len[c] = (uint32_t)(off[c + 1] - off[c]);
  clus[c] = (uint32_t)c;
}

// grid: ceil(k / G) * ns waves, G = clusters per wave (64 / dpad, 1 from d = 64 on), ns = slices
// of 64 dimensions.  lw = log2 of the lanes one cluster takes (6 when G = 1).
__global__ __launch_bounds__(64) void k_km_accumulate(const float* __restrict__ x, int d, int k, int lw, int ns,
                                                      const uint32_t* __restrict__ order,
                                                      const int64_t* __restrict__ off,
                                                      const uint32_t* __restrict__ rows,
                                                      double* __restrict__ sum, int64_t* __restrict__ cnt) {
  constexpr int B = kKmBatch;
  const int lane = threadIdx.x;
  const int grp = blockIdx.x / ns, sl = blockIdx.x - grp * ns;
  const int64_t rank = ((int64_t)grp << (6 - lw)) + (lane >> lw);
  const int t = sl * 64 + (lane & ((1 << lw) - 1));
  if (rank >= k || t >= d) return;
  const uint32_t c = order[rank];
  const int64_t b = off[c], len = off[c + 1] - b;
  if (len == 0) return;  // (and every cluster behind it in `order`)
  const uint32_t* __restrict__ rp = rows + b;
  const float* __restrict__ xt = x + t;
  double* out = sum + (size_t)c * d + t;
  double acc = *out;
  int64_t j = 0;
  uint32_t r[B];
  if (len >= B) {
#pragma unroll
    for (int u = 0; u < B; u++) r[u] = rp[u];
  }
  for (; j + B <= len; j += B) {
    float v[B];
#pragma unroll
    for (int u = 0; u < B; u++) v[u] = xt[(size_t)r[u] * d];
    if (j + 2 * B <= len) {
#pragma unroll
      for (int u = 0; u < B; u++) r[u] = rp[j + B + u];
    }
#pragma unroll
    for (int u = 0; u < B; u++) acc += (double)v[u];
  }
  for (; j < len; j++) acc += (double)xt[(size_t)rp[j] * d];
  *out = acc;
  if (t == 0) cnt[c] += len;
}

// 256 values of the workgroup's threads to thread 0, in a fixed tree
__device__ __forceinline__ double block_tree_sum(double v, double* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) sh[tid] += sh[tid + w];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(256) void k_km_obj_part(const float* __restrict__ D, int64_t n, double* __restrict__ part) {
  __shared__ double sh[256];
  const int64_t i0 = (int64_t)blockIdx.x * kKmObjBlock + threadIdx.x;
  double v = 0.0;
#pragma unroll
  for (int u = 0; u < kKmObjBlock / 256; u++) {
    const int64_t i = i0 + (int64_t)u * 256;
    if (i < n) v += (double)D[i];
  }
  v = block_tree_sum(v, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

__global__ __launch_bounds__(256) void k_km_obj_final(const double* __restrict__ part, int64_t np, double* obj) {
  __shared__ double sh[256];
  double v = 0.0;
  for (int64_t i = threadIdx.x; i < np; i += 256) v += part[i];
  v = block_tree_sum(v, sh);
  if (threadIdx.x == 0) *obj += v;
}

__global__ __launch_bounds__(256) void k_km_mean(const double* __restrict__ sum, const int64_t* __restrict__ cnt,
                                                 int64_t kd, int d, float* __restrict__ cent) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= kd) return;
  const int64_t n = cnt[i / d];
  if (n > 0) cent[i] = (float)(sum[i] / (double)n);
}

__global__ __launch_bounds__(256) void k_km_gather_rows(const float* __restrict__ x, int d, const int64_t* __restrict__ idx,
                                                        int64_t kd, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= kd) return;
  const int64_t c = i / d;
  out[i] = x[idx[c] * d + (i - c * d)];
}

size_t up256(size_t b) { return (b + 255) / 256 * 256; }

size_t km_sort_bytes(int64_t rows, int k) {
  size_t t1 = 0, t2 = 0;
  (void)rocprim::radix_sort_pairs(nullptr, t1, (const uint32_t*)nullptr, (uint32_t*)nullptr, (const uint32_t*)nullptr,
                                  (uint32_t*)nullptr, (size_t)rows, 0, key_bits(k));
  (void)rocprim::radix_sort_pairs_desc(nullptr, t2, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                       (const uint32_t*)nullptr, (uint32_t*)nullptr, (size_t)k, 0, 32);
  return std::max(t1, t2);
}

}  // namespace

size_t km_pass_scratch_bytes(int64_t rows, int k, int64_t tail_rows) {
  return 4 * up256(4 * (size_t)rows) + up256(8 * ((size_t)k + 1)) + 4 * up256(4 * (size_t)k) +
         up256(8 * (size_t)nblk(rows, kKmObjBlock)) +
         up256(std::max(km_sort_bytes(rows, k), km_sort_bytes(std::max<int64_t>(tail_rows, 1), k)));
}

KmPassScratch km_pass_scratch(void* base, int64_t rows, int k, int64_t tail_rows) {
  KmPassScratch w;
  char* p = static_cast<char*>(base);
  auto take = [&](size_t bytes) {
    void* q = p;
    p += up256(bytes);
    return q;
  };
  w.key = (uint32_t*)take(4 * (size_t)rows);
  w.key2 = (uint32_t*)take(4 * (size_t)rows);
  w.row = (uint32_t*)take(4 * (size_t)rows);
  w.row2 = (uint32_t*)take(4 * (size_t)rows);
  w.off = (int64_t*)take(8 * ((size_t)k + 1));
  w.len = (uint32_t*)take(4 * (size_t)k);
  w.len2 = (uint32_t*)take(4 * (size_t)k);
  w.clus = (uint32_t*)take(4 * (size_t)k);
  w.order = (uint32_t*)take(4 * (size_t)k);
  w.part = (double*)take(8 * (size_t)nblk(rows, kKmObjBlock));
  w.sort_bytes = std::max(km_sort_bytes(rows, k), km_sort_bytes(std::max<int64_t>(tail_rows, 1), k));
  w.sort_tmp = take(w.sort_bytes);
  return w;
}

hipError_t launch_km_pass(const float* x, int64_t rows, int d, int k, const int64_t* assign, const float* D,
                          const KmPassScratch& w, double* sum, int64_t* cnt, double* obj, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  // (a ragged last pass sorts fewer rows than the scratch was cut for: its need is checked)
  if (km_sort_bytes(rows, k) > w.sort_bytes) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_km_keys, dim3(nblk(rows, 256)), dim3(256), 0, s, assign, rows, k, w.key, w.row);
  size_t tmp = w.sort_bytes;
  hipError_t e = rocprim::radix_sort_pairs(w.sort_tmp, tmp, w.key, w.key2, w.row, w.row2, (size_t)rows, 0, key_bits(k), s);
  if (e != hipSuccess) return e;
  launch_list_offsets(w.key2, rows, k, w.off, s);
  // the clusters longest first (stable: equal counts in ascending cluster order)
  hipLaunchKernelGGL(k_km_lens, dim3(nblk(k, 256)), dim3(256), 0, s, w.off, k, w.len, w.clus);
  tmp = w.sort_bytes;
  e = rocprim::radix_sort_pairs_desc(w.sort_tmp, tmp, w.len, w.len2, w.clus, w.order, (size_t)k, 0, 32, s);
  if (e != hipSuccess) return e;
  int lw = 6;
  if (d < 64) {
    lw = 0;
    while ((1 << lw) < d) lw++;
  }
  const int ns = (d + 63) / 64;
  const int64_t groups = ((int64_t)k + (64 >> lw) - 1) / (64 >> lw);
  hipLaunchKernelGGL(k_km_accumulate, dim3((unsigned)(groups * ns)), dim3(64), 0, s, x, d, k, lw, ns, w.order, w.off,
                     w.row2, sum, cnt);
  const int64_t np = nblk(rows, kKmObjBlock);
  hipLaunchKernelGGL(k_km_obj_part, dim3((unsigned)np), dim3(256), 0, s, D, rows, w.part);
  hipLaunchKernelGGL(k_km_obj_final, dim3(1), dim3(256), 0, s, w.part, np, obj);
  return hipGetLastError();
}

void launch_km_mean(const double* sum, const int64_t* cnt, int k, int d, float* cent, hipStream_t s) {
  const int64_t kd = (int64_t)k * d;
  hipLaunchKernelGGL(k_km_mean, dim3(nblk(kd, 256)), dim3(256), 0, s, sum, cnt, kd, d, cent);
}

void launch_km_gather_rows(const float* x, int d, const int64_t* idx, int k, float* out, hipStream_t s) {
  const int64_t kd = (int64_t)k * d;
  hipLaunchKernelGGL(k_km_gather_rows, dim3(nblk(kd, 256)), dim3(256), 0, s, x, d, idx, kd, out);
}

}  // namespace chivf
