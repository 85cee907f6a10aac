// gfx950 (MI355X, CDNA4) kernels for the flat product quantizer with 4-bit codes
// (IndexPQ, nbits = 4): Faiss's generic-width IndexPQ at ksub = 16.
//
// The arithmetic is pq_flat.hip's -- per query one M x 16 table in Faiss's fvec order, every
// code summed from M table entries as 0 + t[0] + t[1] + ... in ascending m in fp32, the k
// best by (key, label) -- but a 16-entry sub-table changes how the work is split:
//  * a sub-quantizer of four queries is a 256-byte window of LDS, one float4 per centroid.
//    A ds_read_b128 is served sixteen lanes at a time and the window's sixteen float4 cover
//    the 64 banks once, so lanes with equal nibbles broadcast and lanes with different
//    nibbles never share a bank: the look-up is conflict-free whatever the codes are;
//  * k_pq_scan4 takes four queries per workgroup for every k, one window per sub-quantizer,
//    [m][j][4 queries]; one nibble extract feeds four sums.  Eight queries as two windows
//    side by side were built and measured 1.48 x slower at k <= 64 and are not
//    kept; above 64 the top-k state is 2R registers per query;
//  * 128 sub-quantizers of table are 32 KiB and stay resident for
//    the whole code range; M = 160 ... 256 takes two blocks (128, then the rest) in ascending
//    m with the partial sums kept in registers.  The table's LDS is sized by M at launch, so
//    that M = 32 leaves room for more workgroups per CU;
//  * code rows are M / 2 bytes, read as one uint4 per 32 sub-quantizers and row, the loads of
//    a pass's rows first; rows past the range re-read its last row.  With the 32 look-ups of
//    a uint4 unrolled the sub-table is an immediate offset of the LDS read.
// The wave top-k, admission, queue drains and the sorted write are scan_topk.h's, and the
// partial lists go to launch_merge_topk as the 8-bit scan's do.
// Compiled with -ffp-contract=off like the rest of the library.
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "fvec_tree.h"
#include "pq_flat4.h"
#include "scan_topk.h"

namespace chivf {

namespace {

constexpr int kMaxDsub4 = 64;  // d <= 2048 and M >= 32

// ------------------------------------------------------------------ L2 table
// A workgroup takes (8 queries, 16 sub-quantizers): thread t holds entry (m0 + t / 16, t % 16),
// reads its codeword from memory and the query slices from LDS (the sixteen lanes of a
// sub-quantizer read one address), and writes 256 consecutive floats per query.
constexpr int kTabQ = 8;
constexpr int kTabM = 16;

__global__ __launch_bounds__(256) void k_l2_table4(const float* __restrict__ x, int64_t n, int d,
                                                   const float* __restrict__ cb, int M, float* __restrict__ out) {
  __shared__ float xs[kTabQ * kTabM * kMaxDsub4];
  const int dsub = d / M;
  const int tid = threadIdx.x;
  const int mblocks = M / kTabM;
  const int64_t q0 = (int64_t)(blockIdx.x / mblocks) * kTabQ;
  const int m0 = (blockIdx.x % mblocks) * kTabM;
  const int w = kTabM * dsub;  // floats of a query's slice
  for (int i = tid; i < kTabQ * w; i += 256) {
    const int qq = i / w;
    xs[i] = q0 + qq < n ? x[(q0 + qq) * d + m0 * dsub + (i - qq * w)] : 0.f;
  }
  __syncthreads();
  const float* cw = cb + ((int64_t)m0 * kPq4Ksub + tid) * dsub;  // codeword (m0 + tid / 16, tid % 16)
  const int nqq = (int)min<int64_t>(kTabQ, n - q0);
  for (int qq = 0; qq < nqq; qq++) {
    const float* xq = xs + qq * w + (tid >> 4) * dsub;
    const float v = tree<K_L2>([&](int t) { return xq[t]; }, [&](int t) { return cw[t]; }, dsub);
    out[((q0 + qq) * M + m0) * kPq4Ksub + tid] = v;
  }
}

// ---------------------------------------------------------------- encode
// A workgroup takes 16 sub-quantizers (8 code bytes) of kEncRows rows: their 16 x 16 codewords
// are staged in LDS once (a sub-quantizer's block padded by one float, so that the eight
// byte lanes of a row start on different banks), then thread (row t / 8, byte t % 8) finds
// both nibbles of its byte and writes it, so no two threads write one byte.
constexpr int kEncM = 16;
constexpr int kEncRows = 256;

__global__ __launch_bounds__(256) void k_pq_encode4(const float* __restrict__ x, int64_t n, int d,
                                                    const float* __restrict__ cb, int M,
                                                    uint8_t* __restrict__ codes) {
  __shared__ float cbs[kEncM * (kPq4Ksub * kMaxDsub4 + 1)];
  const int dsub = d / M;
  const int tid = threadIdx.x;
  const int slices = M / kEncM;
  const int m0 = (blockIdx.x % slices) * kEncM;
  const int64_t row0 = (int64_t)(blockIdx.x / slices) * kEncRows;
  const int64_t row1 = min(n, row0 + kEncRows);
  const int per = kPq4Ksub * dsub;  // floats of a sub-quantizer
  const int stride = per + 1;
  for (int i = tid; i < kEncM * per; i += 256) {
    const int mm = i / per;
    cbs[mm * stride + (i - mm * per)] = cb[(int64_t)m0 * per + i];
  }
  __syncthreads();
  const int b = tid & 7;
  for (int64_t row = row0 + (tid >> 3); row < row1; row += 32) {
    uint32_t byte = 0;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const int mm = 2 * b + h;
      const float* xi = x + row * d + (m0 + mm) * dsub;
      const float* cm = cbs + mm * stride;
      uint32_t best = 0;
      float bd = 0.f;
      for (int j = 0; j < kPq4Ksub; j++) {
        const float* cw = cm + j * dsub;
        const float dd = tree<K_L2>([&](int u) { return xi[u]; }, [&](int u) { return cw[u]; }, dsub);
        if (j == 0 || dd < bd) {
          bd = dd;
          best = (uint32_t)j;
        }
      }
      byte |= best << (4 * h);
    }
    codes[row * (M >> 1) + (m0 >> 1) + b] = (uint8_t)byte;
  }
}

// ------------------------------------------------------------------- scan
constexpr int kG4 = 4;              // queries per workgroup: one 256-byte window per sub-quantizer
constexpr int kBlk4 = 128;          // sub-quantizers per table block
constexpr int kRpt4 = 4;            // rows per thread and pass: the queue's pushes per lane and pass
constexpr int kQ4 = kQueue<kRpt4>;  // queued candidates per (wave, query)

// Grid (code ranges, query groups).  Dynamic LDS: the table block, min(M, 128) * 256 bytes,
// as [m][16] float4; static: 40 KiB of candidate queues when R > 1.
// Two waves per SIMD are asked for at R = 1, so that the scheduler does not hoist the
// unrolled look-ups of a piece past 256 registers.
template <int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(R == 1 ? 2 : 1, 2))) void k_pq_scan4(
    const float* __restrict__ tab, int64_t nq, const uint8_t* __restrict__ codes, int64_t nb, int M, int k, int ip,
    int64_t rows, float* __restrict__ partD, int64_t* __restrict__ partI) {
  constexpr int G = kG4;
  constexpr int RPT = kRpt4;
  constexpr bool kQueued = R > 1;
  extern __shared__ float4 lut[];
  float* qd = nullptr;
  int* qi = nullptr;
  if constexpr (kQueued) {
    __shared__ float qd_s[kPqWaves * G * kQ4];
    __shared__ int qi_s[kPqWaves * G * kQ4];
    qd = qd_s;
    qi = qi_s;
  }
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int64_t q0 = (int64_t)blockIdx.y * G;
  const int64_t r0 = (int64_t)blockIdx.x * rows;
  const int64_t r1 = min(nb, r0 + rows);
  if (r0 >= r1) return;  // uniform (the host launches no empty range)
  const int row_bytes = M >> 1;
  const int nblk = (M + kBlk4 - 1) / kBlk4;

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
    // rows past the range re-read its last row (their sums are dropped below)
    const uint8_t* src[RPT];
#pragma unroll
    for (int i = 0; i < RPT; i++) src[i] = codes + min(t0 + i * 256 + tid, r1 - 1) * row_bytes;

    for (int b = 0; b < nblk; b++) {
      const int m0 = b * kBlk4;
      const int mb = min(kBlk4, M - m0);
      if (nblk > 1 || t0 == r0) {  // a table of one block stays resident for the whole range
        __syncthreads();           // the previous block's reads are done
        for (int e = tid; e < mb * kPq4Ksub; e += 256) {  // entry (m0 + e / 16, e % 16) of every query
          float c[G];
#pragma unroll
          for (int g = 0; g < G; g++) {
            // queries past the batch read the last one's table (their lists are not written)
            const int64_t q = min(q0 + g, nq - 1);
            const float t = tab[(q * M + m0) * kPq4Ksub + e];
            c[g] = ip ? -t : t;
          }
          lut[e] = make_float4(c[0], c[1], c[2], c[3]);
        }
        __syncthreads();
      }
      // the block in pieces of 32 sub-quantizers: one uint4 of every row of the pass, then its look-ups
      const int np = mb >> 5;
      for (int p = 0; p < np; p++) {
        uint32_t cw[RPT][4];
#pragma unroll
        for (int i = 0; i < RPT; i++) {
          const uint4 u = *reinterpret_cast<const uint4*>(src[i] + ((m0 + p * 32) >> 1));
          cw[i][0] = u.x, cw[i][1] = u.y, cw[i][2] = u.z, cw[i][3] = u.w;
        }
        const float4* lp = lut + p * 32 * kPq4Ksub;
#pragma unroll
        for (int mm = 0; mm < 32; mm++) {
#pragma unroll
          for (int i = 0; i < RPT; i++) {
            const uint32_t c = (cw[i][mm >> 3] >> (4 * (mm & 7))) & 15u;
            const float4 v = lp[mm * kPq4Ksub + c];
            acc[i][0] = acc[i][0] + v.x;
            acc[i][1] = acc[i][1] + v.y;
            acc[i][2] = acc[i][2] + v.z;
            acc[i][3] = acc[i][3] + v.w;
          }
        }
      }
    }

    // admission against each query's running k-th best
#pragma unroll
    for (int i = 0; i < RPT; i++) {
      const int64_t row = t0 + i * 256 + tid;
#pragma unroll
      for (int g = 0; g < G; g++)
        admit<R>(tk[g], row < r1, acc[i][g], (int)row, qn[g], kQueued ? qd + (wave * G + g) * kQ4 : nullptr,
                 kQueued ? qi + (wave * G + g) * kQ4 : nullptr, lane);
    }
    if constexpr (kQueued)
      drain_queues<kRpt4, false>(tk, qn, t0 + 256 * RPT < r1 ? 63 : 0, qd, qi, wave, lane, nullptr, nullptr);
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

template <int R>
void launch_scan4_R(const float* tab, int64_t nq, const uint8_t* codes, int64_t nb, int M, int k, bool ip,
                    const PqScanPlan& p, float* partD, int64_t* partI, hipStream_t s) {
  const dim3 grid((unsigned)p.ranges, nblocks(nq, kG4));
  const size_t lds = (size_t)std::min(M, kBlk4) * kPq4Ksub * sizeof(float4);
  hipLaunchKernelGGL(k_pq_scan4<R>, grid, dim3(256), lds, s, tab, nq, codes, nb, M, k, ip ? 1 : 0, p.rows, partD,
                     partI);
}

}  // namespace

bool pq_flat4_supported_M(int M) { return M >= 32 && M <= 256 && M % 32 == 0; }

void launch_l2_table4(const float* x, int64_t n, int d, const float* cb, int M, float* out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_l2_table4, dim3(nblocks(n, kTabQ) * (unsigned)(M / kTabM)), dim3(256), 0, s, x, n, d, cb, M,
                     out);
}

void launch_pq_encode4(const float* x, int64_t n, int d, const float* cb, int M, uint8_t* codes, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_pq_encode4, dim3(nblocks(n, kEncRows) * (unsigned)(M / kEncM)), dim3(256), 0, s, x, n, d, cb, M,
                     codes);
}

PqScanPlan pq_scan4_plan(int k, int64_t nq, int64_t nb) { return pq_scan_plan_group(kG4, k, nq, nb); }

void launch_pq_scan4(const float* tab, int64_t nq, const uint8_t* codes, int64_t nb, int M, int k, bool ip,
                     const PqScanPlan& p, float* partD, int64_t* partI, hipStream_t s) {
  if (nq <= 0 || nb <= 0) return;
  switch (scan_rows_for(k)) {
    case 1: launch_scan4_R<1>(tab, nq, codes, nb, M, k, ip, p, partD, partI, s); break;
    case 4: launch_scan4_R<4>(tab, nq, codes, nb, M, k, ip, p, partD, partI, s); break;
    default: launch_scan4_R<16>(tab, nq, codes, nb, M, k, ip, p, partD, partI, s); break;
  }
}

}  // namespace chivf
