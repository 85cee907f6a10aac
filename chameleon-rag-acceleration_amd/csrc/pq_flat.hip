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
//    (the bitonic wave top-k of ivfpq_kernels.hip, restated here for int32
//    positions) and writes them sorted; launch_merge_topk merges the partial lists.
//    k <= 64 merges a pass's admitted rows at once (admissions are rare: ~k ln(n / k)
//    per wave); k > 64, where a merge costs R = k / 64 rows of bitonic network and
//    most early passes admit something, queues admitted rows in LDS per (wave, query)
//    and merges 64 at a time.
// Compiled with -ffp-contract=off like the rest of the library.
#include <float.h>
#include <stdint.h>

#include <algorithm>

#include <hip/hip_runtime.h>

#include "pq_flat.h"

namespace chivf {

namespace {

constexpr float kInf = __builtin_huge_valf();
constexpr int kNone = INT32_MAX;  // "no candidate" position (real positions are < 2^31 - 1)

enum { K_IP = 0, K_L2 = 1 };

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

// ---- wave top-k in registers (int32 positions) ---------------------------------
__device__ __forceinline__ bool lexless(float ad, int ai, float bd, int bi) {
  return (ad < bd) | ((ad == bd) & (ai < bi));
}
__device__ __forceinline__ float readlane_f(float v, int lane) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
template <int CTRL>
__device__ __forceinline__ int dmov(int v) {
  return __builtin_amdgcn_mov_dpp(v, CTRL, 0xf, 0xf, false);
}
// lane ^ J exchange on the VALU: DPP for J <= 8, the gfx950 row / half swaps above
template <int J>
__device__ __forceinline__ int xor_i(int v) {
  if constexpr (J == 1) return dmov<0xB1>(v);
  else if constexpr (J == 2) return dmov<0x4E>(v);
  else if constexpr (J == 4) return dmov<0x1B>(dmov<0x141>(v));
  else if constexpr (J == 8) return dmov<0x128>(v);
  else if constexpr (J == 16) {
    const auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
    return (int)((__lane_id() & 16) ? r[0] : r[1]);
  } else {
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
    return (int)((__lane_id() & 32) ? r[0] : r[1]);
  }
}
template <int J>
__device__ __forceinline__ float xor_f(float v) { return __int_as_float(xor_i<J>(__float_as_int(v))); }
__device__ __forceinline__ int rev64_i(int v) { return xor_i<16>(xor_i<32>(dmov<0x140>(v))); }
__device__ __forceinline__ float rev64_f(float v) { return __int_as_float(rev64_i(__float_as_int(v))); }

// A wave's running k best (key, position) pairs, sorted ascending across R rows x 64
// lanes (logical index r * 64 + lane); k <= 64 * R.
template <int R>
struct WaveTopK {
  float d[R];
  int id[R];
  float td;  // current k-th best (the admission threshold)
  int ti;
  int krow, klane;

  __device__ __forceinline__ void init(int k) {
#pragma unroll
    for (int r = 0; r < R; r++) {
      d[r] = kInf;
      id[r] = kNone;
    }
    td = kInf;
    ti = kNone;
    krow = (k - 1) >> 6;
    klane = (k - 1) & 63;
  }
  __device__ __forceinline__ void refresh_tau() {
#pragma unroll
    for (int r = 0; r < R; r++) {
      if (r == krow) {
        td = readlane_f(d[r], klane);
        ti = __builtin_amdgcn_readlane(id[r], klane);
      }
    }
  }
};

template <int KK, int J>
__device__ __forceinline__ void bitonic_step(float& cd, int& ci, int lane) {
  const float od = xor_f<J>(cd);
  const int oi = xor_i<J>(ci);
  const bool want_min = ((lane & J) == 0) == ((lane & KK) == 0);
  const bool o_lt = lexless(od, oi, cd, ci);
  const bool c_lt = lexless(cd, ci, od, oi);
  const bool take = (want_min & o_lt) | (!want_min & c_lt);
  cd = take ? od : cd;
  ci = take ? oi : ci;
}
template <int KK, int J>
__device__ __forceinline__ void bitonic_steps(float& cd, int& ci, int lane) {
  if constexpr (J >= 1) {
    bitonic_step<KK, J>(cd, ci, lane);
    bitonic_steps<KK, J / 2>(cd, ci, lane);
  }
}
template <int KK>
__device__ __forceinline__ void bitonic_sort64(float& cd, int& ci, int lane) {
  if constexpr (KK <= 64) {
    bitonic_steps<KK, KK / 2>(cd, ci, lane);
    bitonic_sort64<KK * 2>(cd, ci, lane);
  }
}

// Merge up to 64 candidates (one per lane; (inf, none) = no candidate) into the R-row
// top-k: bitonic sort of the candidates, then per row the reverse-min + bitonic merge,
// the upper half carried to the next row.
template <int R>
__device__ __forceinline__ void bulk_merge_rows(WaveTopK<R>& tk, float cd, int ci, int lane) {
  bitonic_sort64<2>(cd, ci, lane);
#pragma unroll
  for (int r = 0; r < R; r++) {
    const float rd = rev64_f(cd);
    const int ri = rev64_i(ci);
    const bool t = lexless(rd, ri, tk.d[r], tk.id[r]);
    const float lo_d = t ? rd : tk.d[r], hi_d = t ? tk.d[r] : rd;
    const int lo_i = t ? ri : tk.id[r], hi_i = t ? tk.id[r] : ri;
    tk.d[r] = lo_d;
    tk.id[r] = lo_i;
    bitonic_steps<128, 32>(tk.d[r], tk.id[r], lane);  // KK = 128: every lane ascending
    if (r + 1 < R) {
      cd = hi_d;
      ci = hi_i;
      bitonic_steps<128, 32>(cd, ci, lane);
    }
  }
  tk.refresh_tau();
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

__global__ __launch_bounds__(256) void k_pq_fill_empty(float* __restrict__ D, int64_t* __restrict__ I, int64_t n,
                                                       float pad) {
  const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (gid >= n) return;
  D[gid] = pad;
  I[gid] = -1;
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
constexpr int kQueue = 64 + kRptQ * 64;   // queued candidates per (wave, query): < 64 pending + a pass's pushes

// The first min(n, 64) candidates of a wave's queue (q_d, q_i) into its top-k, the
// rest moved to the front; n becomes the number left.
template <int R>
__device__ __forceinline__ void drain_queue(WaveTopK<R>& tk, int& n, float* q_d, int* q_i, int lane) {
  __builtin_amdgcn_wave_barrier();
  const bool have = lane < n;
  const float cd = have ? q_d[lane] : kInf;
  const int ci = have ? q_i[lane] : kNone;
  const int rem = max(n - 64, 0);
  float md[kRptQ];
  int mi[kRptQ];
#pragma unroll
  for (int j = 0; j < kRptQ; j++) {
    const bool mv = j * 64 + lane < rem;
    md[j] = mv ? q_d[64 + j * 64 + lane] : kInf;
    mi[j] = mv ? q_i[64 + j * 64 + lane] : kNone;
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < kRptQ; j++) {
    if (j * 64 + lane < rem) {
      q_d[j * 64 + lane] = md[j];
      q_i[j * 64 + lane] = mi[j];
    }
  }
  __builtin_amdgcn_wave_barrier();
  n = rem;
  const bool pass = lexless(cd, ci, tk.td, tk.ti);  // the bound may have moved since the push
  if (__ballot(pass)) bulk_merge_rows<R>(tk, pass ? cd : kInf, pass ? ci : kNone, lane);
}

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
  __shared__ float qd[kQueued ? kPqWaves * G * kQueue : 1];
  __shared__ int qi[kQueued ? kPqWaves * G * kQueue : 1];
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

    // admission against each query's running k-th best; a pass with no better row
    // costs one compare and one ballot per (row, query)
#pragma unroll
    for (int i = 0; i < RPT; i++) {
      const int64_t row = t0 + i * 256 + tid;
      const bool valid = row < r1;
#pragma unroll
      for (int g = 0; g < G; g++) {
        const bool pass = valid & lexless(acc[i][g], (int)row, tk[g].td, tk[g].ti);
        const uint64_t mask = __ballot(pass);
        if (!mask) continue;
        if constexpr (!kQueued) {
          bulk_merge_rows<R>(tk[g], pass ? acc[i][g] : kInf, pass ? (int)row : kNone, lane);
        } else {
          const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
          if (pass) {
            const int slot = (wave * G + g) * kQueue + qn[g] + before;
            qd[slot] = acc[i][g];
            qi[slot] = (int)row;
          }
          qn[g] += __popcll(mask);
        }
      }
    }
    if constexpr (kQueued) {
      // one drain site per query: full batches of 64 after every pass, the rest after the last
      const int keep = t0 + 256 * RPT < r1 ? 63 : 0;
      // (spelled out per query: a loop over g around R = 16 merges is past the
      // compiler's unroll budget, and the top-k arrays would then live in scratch)
      static_assert(G <= 4, "drain sites are spelled out for up to four queries");
#define PQ_DRAIN(g)                                                                                       \
  if constexpr (G > g)                                                                                    \
    while (qn[g] > keep)                                                                                  \
      drain_queue<R>(tk[g], qn[g], qd + (wave * G + g) * kQueue, qi + (wave * G + g) * kQueue, lane)
      PQ_DRAIN(0);
      PQ_DRAIN(1);
      PQ_DRAIN(2);
      PQ_DRAIN(3);
#undef PQ_DRAIN
    }
  }

  const int64_t part = (int64_t)blockIdx.x * kPqWaves + wave;
#pragma unroll
  for (int g = 0; g < G; g++) {
    if (q0 + g >= nq) continue;
    const int64_t base = (part * nq + (q0 + g)) * k;
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int idx = r * 64 + lane;
      if (idx < k) {
        const bool none = tk[g].id[r] == kNone;
        const float key = tk[g].d[r];
        partD[base + idx] = none ? (ip ? -FLT_MAX : FLT_MAX) : (ip ? -key : key);
        partI[base + idx] = none ? -1 : (int64_t)tk[g].id[r];
      }
    }
  }
}

inline unsigned nblocks(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

inline int scan_rows_for(int k) { return k <= 64 ? 1 : k <= 256 ? 4 : 16; }
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

void launch_pq_fill_empty(float* D, int64_t* I, int64_t n, bool ip, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_pq_fill_empty, dim3(nblocks(n, 256)), dim3(256), 0, s, D, I, n, ip ? -FLT_MAX : FLT_MAX);
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
