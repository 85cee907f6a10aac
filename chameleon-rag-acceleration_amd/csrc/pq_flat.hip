// gfx950 (MI355X, CDNA4) kernels for the flat product quantizer (IndexPQ).
//
// Faiss runs IndexPQ::search as pq.compute_distance_tables / compute_inner_prod_tables
// followed by pq_knn_search_with_tables: per query one M x 256 table, then every code
// summed from M table entries in ascending m into a heap.  Here:
//  * the table is launch_ip_table's T3 (inner product) or k_l2_table's |q_m - C_mj|^2
//    (L2), both in Faiss's fvec order (tree<>);
//  * k_pq_scan is query-major: a workgroup takes G queries and a contiguous range of
//    code rows, holds the G tables in LDS interleaved [m][j][g] (one code byte = one
//    LDS read for all G queries) and streams the rows behind them; tables larger
//    than the LDS block are taken in blocks of MB sub-quantizers in ascending m with
//    the partial sums kept in registers, so every sum is 0 + t[0] + t[1] + ... in
//    Faiss's order whatever the blocking;
//  * each wave keeps the k best (key, position) of the rows it summed in registers
//    (the wave top-k of scan_topk.h, shared with the exact scans; this scan has no
//    shared bound) and writes them sorted; launch_merge_topk merges the partial lists.
//    k <= 64 merges a pass's admitted rows at once (admissions are rare: ~k ln(n / k)
//    per wave); k > 64, where a merge costs R = k / 64 rows of bitonic network and
//    most early passes admit something, queues admitted rows in LDS per (wave, query)
//    and merges 64 at a time.  Admission, drain sites and the sorted write are
//    scan_topk.h's, with a queue of kRptQ pushes per lane and pass.
// Compiled with -ffp-contract=off like the rest of the library.
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "pq_flat.h"
#include "scan_topk.h"

namespace chivf {

namespace {

// Faiss-1.7.1 AVX reduction order (or_tree in oracle/ivfpq_oracle.c; the same
// function as tree<> in ivfpq_kernels.hip).
template <int KIND, class FX, class FY>
__device__ __forceinline__ float tree(FX fx, FY fy, int d) {
  float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int i = 0;
  for (; i + 8 <= d; i += 8) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      float p;
      if (KIND == K_IP) {
        p = fx(i + j) * fy(i + j);
      } else {
        float t = fx(i + j) - fy(i + j);
        p = t * t;
      }
      a8[j] = a8[j] + p;
    }
  }
  float a4[4];
#pragma unroll
  for (int j = 0; j < 4; j++) a4[j] = a8[j + 4] + a8[j];
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
    // pass 0: the 4-wide remainder (d - i >= 4); pass 1: the masked tail
    if (pass == 0 && i + 4 > d) continue;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      if (i + j < d) {
        float p;
        if (KIND == K_IP) {
          p = fx(i + j) * fy(i + j);
        } else {
          float t = fx(i + j) - fy(i + j);
          p = t * t;
        }
        a4[j] = a4[j] + p;
      }
    }
    if (pass == 0) i += 4;
  }
  float h0 = a4[0] + a4[1];
  float h1 = a4[2] + a4[3];
  return h0 + h1;
}

// ------------------------------------------------------------------ L2 table
// k_ip_tiles' tiling: a workgroup takes (16 queries, sub-quantizer m), thread t holds
// codeword (m, t) and writes entry (q, m, t) of the 16 queries, coalesced over t.
// DSUB = 0: runtime dsub (<= 256), the codeword read from memory.
constexpr int GQ = 16;

template <int DSUB>
__global__ __launch_bounds__(256) void k_l2_table(const float* __restrict__ x, int64_t n, int d,
                                                  const float* __restrict__ cb, int M, float* __restrict__ out) {
  constexpr int XS = DSUB ? DSUB : 256;
  __shared__ float xs[GQ * XS];
  const int dsub = DSUB ? DSUB : d / M;
  const int tid = threadIdx.x;
  const int64_t q0 = (int64_t)(blockIdx.x / M) * GQ;
  const int m = blockIdx.x % M;
  for (int i = tid; i < GQ * dsub; i += 256) {
    const int qq = i / dsub;
    xs[i] = q0 + qq < n ? x[(q0 + qq) * d + m * dsub + (i - qq * dsub)] : 0.f;
  }
  const float* src = cb + ((int64_t)m * 256 + tid) * dsub;
  float cw[DSUB ? DSUB : 1];
  if constexpr (DSUB > 0) {
#pragma unroll
    for (int t = 0; t < DSUB; t++) cw[t] = src[t];
  }
  __syncthreads();
  const int64_t total = (int64_t)M * 256;
  const int nqq = (int)min<int64_t>(GQ, n - q0);
  for (int qq = 0; qq < nqq; qq++) {
    const float* xq = xs + qq * dsub;
    float v;
    if constexpr (DSUB > 0)
      v = tree<K_L2>([&](int t) { return xq[t]; }, [&](int t) { return cw[t]; }, DSUB);
    else
      v = tree<K_L2>([&](int t) { return xq[t]; }, [&](int t) { return src[t]; }, dsub);
    out[(q0 + qq) * total + m * 256 + tid] = v;
  }
}

// ---------------------------------------------------------------- encode
__global__ __launch_bounds__(256) void k_pq_encode_flat(const float* __restrict__ x, int64_t n, int d,
                                                        const float* __restrict__ cb, int M,
                                                        uint8_t* __restrict__ codes) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n * M) return;
  const int m = (int)(gid % M);
  const int64_t i = gid / M;
  const int dsub = d / M;
  const float* xi = x + i * d + m * dsub;
  int best = 0;
  float bd = 0.f;
  for (int j = 0; j < 256; j++) {
    const float* cw = cb + ((int64_t)m * 256 + j) * dsub;
    const float dd = tree<K_L2>([&](int u) { return xi[u]; }, [&](int u) { return cw[u]; }, dsub);
    if (j == 0 || dd < bd) {
      bd = dd;
      best = j;
    }
  }
  codes[gid] = (uint8_t)best;
}

// ------------------------------------------------------------------- scan
template <int G>
struct LutVec;
template <>
struct LutVec<4> {
  using type = float4;
};
__device__ __forceinline__ float comp(float4 v, int g) { return g == 0 ? v.x : g == 1 ? v.y : g == 2 ? v.z : v.w; }
__device__ __forceinline__ void setc(float4& o, int g, float x) {
  if (g == 0) o.x = x; else if (g == 1) o.y = x; else if (g == 2) o.z = x; else o.w = x;
}

constexpr int kRpt = kPqTileRows / 256;  // rows per thread and pass (k <= 64)
constexpr int kRptQ = 4;                  // the same with candidate queues (k > 64)
constexpr int kQ = kQueue<kRptQ>;        // queued candidates per (wave, query)

// Grid (code ranges, query groups).  MB code bytes (sub-quantizers) per table block:
// 8 (M = 8) or 16; LDS = MB * G KiB, plus 10 * G KiB of candidate queues when R > 1.
template <int G, int R, int MB, int RPT>
__global__ __launch_bounds__(256) void k_pq_scan(const float* __restrict__ tab, int64_t nq,
                                                 const uint8_t* __restrict__ codes, int64_t nb, int M, int k, int ip,
                                                 int64_t rows, float* __restrict__ partD,
                                                 int64_t* __restrict__ partI) {
  using LV = typename LutVec<G>::type;
  constexpr int W = MB / 4;  // 32-bit code words per row and block
  __shared__ LV lut[MB * 256];
  constexpr bool kQueued = R > 1;
  __shared__ float qd[kQueued ? kPqWaves * G * kQ : 1];
  __shared__ int qi[kQueued ? kPqWaves * G * kQ : 1];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.y * G;
  const int64_t r0 = (int64_t)blockIdx.x * rows;
  const int64_t r1 = min(nb, r0 + rows);
  if (r0 >= r1) return;  // uniform (the host launches no empty range)
  const int nblk = M / MB;

  WaveTopK<R> tk[G];
#pragma unroll
  for (int g = 0; g < G; g++) tk[g].init(k);
  int qn[G];  // queue fills (wave-uniform, < 64 between passes)
#pragma unroll
  for (int g = 0; g < G; g++) qn[g] = 0;
  for (int64_t t0 = r0; t0 < r1; t0 += 256 * RPT) {
    float acc[RPT][G];
#pragma unroll
    for (int i = 0; i < RPT; i++)
#pragma unroll
      for (int g = 0; g < G; g++) acc[i][g] = 0.f;

    for (int b = 0; b < nblk; b++) {
      if (nblk > 1 || t0 == r0) {  // a table of one block stays resident for the whole range
        __syncthreads();           // the previous block's reads are done
#pragma unroll 4
        for (int mm = 0; mm < MB; mm++) {
          LV v;
#pragma unroll
          for (int g = 0; g < G; g++) {
            // queries past the batch read the last one's table (their lists are not written)
            const int64_t q = min(q0 + g, nq - 1);
            const float e = tab[(q * M + (b * MB + mm)) * 256 + tid];
            setc(v, g, ip ? -e : e);
          }
          lut[mm * 256 + tid] = v;
        }
        __syncthreads();
      }
      // this block's code bytes of the pass's rows, all loads first; rows past the
      // range re-read its last row (their sums are dropped below)
      uint32_t cw[RPT][W];
#pragma unroll
      for (int i = 0; i < RPT; i++) {
        const int64_t row = min(t0 + i * 256 + tid, r1 - 1);
        const uint8_t* src = codes + row * M + b * MB;
        if constexpr (W == 4) {
          const uint4 u = *reinterpret_cast<const uint4*>(src);
          cw[i][0] = u.x, cw[i][1] = u.y, cw[i][2] = u.z, cw[i][3] = u.w;
        } else {
          const uint2 u = *reinterpret_cast<const uint2*>(src);
          cw[i][0] = u.x, cw[i][1] = u.y;
        }
      }
#pragma unroll
      for (int mm = 0; mm < MB; mm++) {
#pragma unroll
        for (int i = 0; i < RPT; i++) {
          const uint32_t c = (cw[i][mm >> 2] >> (8 * (mm & 3))) & 255u;
          const LV v = lut[mm * 256 + c];
#pragma unroll
          for (int g = 0; g < G; g++) acc[i][g] = acc[i][g] + comp(v, g);
        }
      }
    }

    // admission against each query's running k-th best
#pragma unroll
    for (int i = 0; i < RPT; i++) {
      const int64_t row = t0 + i * 256 + tid;
#pragma unroll
      for (int g = 0; g < G; g++)
        admit<R>(tk[g], row < r1, acc[i][g], (int)row, qn[g], qd + (wave * G + g) * kQ, qi + (wave * G + g) * kQ, lane);
    }
    if constexpr (kQueued)
      drain_queues<kRptQ, false>(tk, qn, t0 + 256 * RPT < r1 ? 63 : 0, qd, qi, wave, lane, nullptr, nullptr);
  }

  // this wave's sorted list of every query; the label of a row is its position
  const int64_t part = (int64_t)blockIdx.x * kPqWaves + wave;
#pragma unroll
  for (int g = 0; g < G; g++) {
    if (q0 + g >= nq) continue;
    const int64_t base = (part * nq + (q0 + g)) * k;
    write_sorted<R>(tk[g], k, ip != 0, partD + base, partI + base, lane, [](int pos) { return (int64_t)pos; });
  }
}

constexpr int kScanGroup = 4;  // queries per workgroup

template <int G, int R>
void launch_scan_GR(const float* tab, int64_t nq, const uint8_t* codes, int64_t nb, int M, int k, bool ip,
                    const PqScanPlan& p, float* partD, int64_t* partI, hipStream_t s) {
  const dim3 grid((unsigned)p.ranges, nblocks(nq, G));
  constexpr int RPT = R > 1 ? kRptQ : kRpt;
  if (M == 8)
    hipLaunchKernelGGL((k_pq_scan<G, R, 8, RPT>), grid, dim3(256), 0, s, tab, nq, codes, nb, M, k, ip ? 1 : 0, p.rows,
                       partD, partI);
  else
    hipLaunchKernelGGL((k_pq_scan<G, R, 16, RPT>), grid, dim3(256), 0, s, tab, nq, codes, nb, M, k, ip ? 1 : 0, p.rows,
                       partD, partI);
}

}  // namespace

bool pq_flat_supported_M(int M) { return M == 8 || (M >= 16 && M <= 128 && M % 16 == 0); }

void launch_l2_table(const float* x, int64_t n, int d, const float* cb, int M, float* out, hipStream_t s) {
  if (n <= 0) return;
  const dim3 grid(nblocks(n, GQ) * (unsigned)M);
  switch (d / M) {
    case 2: hipLaunchKernelGGL(k_l2_table<2>, grid, dim3(256), 0, s, x, n, d, cb, M, out); break;
    case 4: hipLaunchKernelGGL(k_l2_table<4>, grid, dim3(256), 0, s, x, n, d, cb, M, out); break;
    case 8: hipLaunchKernelGGL(k_l2_table<8>, grid, dim3(256), 0, s, x, n, d, cb, M, out); break;
    case 12: hipLaunchKernelGGL(k_l2_table<12>, grid, dim3(256), 0, s, x, n, d, cb, M, out); break;
    case 16: hipLaunchKernelGGL(k_l2_table<16>, grid, dim3(256), 0, s, x, n, d, cb, M, out); break;
    default: hipLaunchKernelGGL(k_l2_table<0>, grid, dim3(256), 0, s, x, n, d, cb, M, out); break;  // dsub <= 256
  }
}

void launch_pq_encode_flat(const float* x, int64_t n, int d, const float* cb, int M, uint8_t* codes, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_pq_encode_flat, dim3(nblocks(n * M, 256)), dim3(256), 0, s, x, n, d, cb, M, codes);
}

// Ranges: enough workgroups for two rounds of two per CU on 256 CUs, but no more
// partial lists than the merge takes cheaply (S * k <= 12288 entries per query).
PqScanPlan pq_scan_plan(int M, int k, int64_t nq, int64_t nb) {
  (void)M;
  PqScanPlan p;
  (void)k;
  p.G = kScanGroup;
  const int64_t groups = (nq + p.G - 1) / p.G;
  const int64_t tiles = std::max<int64_t>(1, (nb + kPqTileRows - 1) / kPqTileRows);
  int64_t ranges = (1024 + groups - 1) / std::max<int64_t>(groups, 1);
  ranges = std::min<int64_t>(ranges, std::max<int64_t>(1, 12288 / ((int64_t)kPqWaves * k)));
  ranges = std::max<int64_t>(1, std::min(ranges, tiles));
  p.rows = (tiles + ranges - 1) / ranges * kPqTileRows;
  p.ranges = (int)std::max<int64_t>(1, (nb + p.rows - 1) / p.rows);
  p.S = p.ranges * kPqWaves;
  return p;
}

void launch_pq_scan(const float* tab, int64_t nq, const uint8_t* codes, int64_t nb, int M, int k, bool ip,
                    const PqScanPlan& p, float* partD, int64_t* partI, hipStream_t s) {
  if (nq <= 0 || nb <= 0) return;
  switch (scan_rows_for(k)) {
    case 1: launch_scan_GR<4, 1>(tab, nq, codes, nb, M, k, ip, p, partD, partI, s); break;
    case 4: launch_scan_GR<4, 4>(tab, nq, codes, nb, M, k, ip, p, partD, partI, s); break;
    default: launch_scan_GR<4, 16>(tab, nq, codes, nb, M, k, ip, p, partD, partI, s); break;
  }
}

}  // namespace chivf
